"""The training step on the MI355X (csrc/optim_f32.hip, k-diffusion_amd/optim.py, utils.py, training.py, train.py): the fused clip +
AdamW + EMA step against torch on the CPU in fp64 (yardstick: torch on the CPU in fp32), its options against the unfused composition of
this project's own calls, the sigma densities against the reference's recorded fp64 outputs, optimizer state interchange with
``torch.optim.AdamW``, the launch plan following the raw-pointer updates, and ``train.py`` end to end with a bit-exact ``--resume``."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = cases.REPO
BETAS, EPS, WD, LR = (0.9, 0.99), 1e-8, 1e-2, 2e-3
# per-step gradient scales: the global norm is far above the clip threshold 1 on some steps and far below it on others
GRAD_SCALES = [3e-1, 1e-5, 2e-1, 3e-6, 1e-1]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _model(KD, name, seed=cases.WEIGHT_SEED):
    cfg = KD.config.load_config(cases.raw_config(name))
    model = KD.config.make_model(cfg)
    model.load_state_dict(KD.synth.synth_state_dict(model.state_dict(), seed=seed))
    return cfg, model


def _group_names(model, lr):
    names = {id(p): n for n, p in model.named_parameters()}
    return [([names[id(p)] for p in grp["params"]], {k: v for k, v in grp.items() if k != "params"}) for grp in model.param_groups(lr)]


def _grads(shapes, step):
    gen = _gen(1000 + step)
    return {n: torch.randn(s, generator=gen) * GRAD_SCALES[step % len(GRAD_SCALES)] for n, s in shapes.items()}


def _ema_decays(KD, n):
    sched = KD.utils.EMAWarmup(power=0.6667, max_value=0.9999)
    out = []
    for _ in range(n):
        out.append(sched.get_value())
        sched.step()
    return out


class _TorchCpu:
    """clip_grad_norm_ + torch.optim.AdamW(foreach=False) + lerp_ on the CPU in ``dtype``, from the same fp32 inputs."""

    def __init__(self, start, groups, dtype):
        self.p = {n: torch.nn.Parameter(t.detach().cpu().to(dtype).clone()) for n, t in start.items()}
        self.ema = {n: t.detach().cpu().to(dtype).clone() for n, t in start.items()}
        self.opt = torch.optim.AdamW([{"params": [self.p[n] for n in names], **kw} for names, kw in groups], lr=LR, betas=BETAS, eps=EPS,
                                     weight_decay=WD, foreach=False)
        self.dtype = dtype
        self.norms = []

    def step(self, grads, decay, clip=1.0):
        for n, p in self.p.items():
            p.grad = grads[n].to(self.dtype).clone()
        if clip is not None:
            self.norms.append(torch.nn.utils.clip_grad_norm_(list(self.p.values()), clip, foreach=False))
        self.opt.step()
        if decay is not None:
            with torch.no_grad():
                for n, p in self.p.items():
                    self.ema[n].lerp_(p, 1 - decay)

    def tensors(self):
        out = {}
        for n, p in self.p.items():
            st = self.opt.state[p]
            out[n] = (p.detach(), st["exp_avg"], st["exp_avg_sq"], self.ema[n])
        return out


class _Hip:
    def __init__(self, KD, start, groups):
        self.p = {n: torch.nn.Parameter(t.detach().to(DEV, torch.float32).clone()) for n, t in start.items()}
        self.ema = {n: torch.nn.Parameter(t.detach().to(DEV, torch.float32).clone()) for n, t in start.items()}
        self.opt = KD.optim.AdamW([{"params": [self.p[n] for n in names], **kw} for names, kw in groups], lr=LR, betas=BETAS, eps=EPS,
                                  weight_decay=WD)
        model, avg = torch.nn.Module(), torch.nn.Module()
        for n in start:
            model.register_parameter(n.replace(".", "_"), self.p[n])
            avg.register_parameter(n.replace(".", "_"), self.ema[n])
        self.opt.attach_ema(model, avg)
        self.model, self.avg = model, avg
        self.norms = []

    def step(self, grads, decay, clip=1.0, **kw):
        for n, p in self.p.items():
            if p.grad is None:
                p.grad = grads[n].to(DEV)
            else:
                p.grad.copy_(grads[n])
        norm = self.opt.step(clip_grad_norm=clip, ema_decay=decay, **kw)
        if clip is not None:
            self.norms.append(norm)

    def tensors(self):
        out = {}
        for n, p in self.p.items():
            st = self.opt.state[p]
            out[n] = (p.detach(), st["exp_avg"], st["exp_avg_sq"], self.ema[n].detach())
        return out


KINDS = ("p", "exp_avg", "exp_avg_sq", "ema")


def _parity(hip, f32, f64, what):
    """Per tensor: max|hip - fp64| <= 4 max|torch fp32 - fp64| (the factor covers another operation order and FMA contraction).  Prints
    the worst ratio per kind."""
    worst, misses = {k: 0.0 for k in KINDS}, []
    for n in f64:
        for kind, a, b, c in zip(KINDS, hip[n], f32[n], f64[n]):
            e_hip = (a.detach().cpu().double() - c).abs().max().item()
            e_ref = (b.detach().double() - c).abs().max().item()
            ratio = e_hip / e_ref if e_ref > 0 else (0.0 if e_hip == 0 else math.inf)
            worst[kind] = max(worst[kind], ratio)
            if not e_hip <= 4 * e_ref:
                misses.append((n, kind, e_hip, e_ref))
    print(f"{what}: worst max|hip - fp64| / max|torch fp32 - fp64| per kind: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not misses, misses[:5]


@pytest.mark.parametrize("name", ["tiny_sw", "tiny_na"])
def test_adamw_clip_ema_parity(KD, name):
    _, model = _model(KD, name)
    start = dict(model.named_parameters())
    groups = _group_names(model, LR)
    shapes = {n: p.shape for n, p in start.items()}
    decays = _ema_decays(KD, 5)

    def run_hip():
        hip = _Hip(KD, start, groups)
        for s in range(5):
            hip.step(_grads(shapes, s), decays[s])
        return hip

    hip = run_hip()
    f32, f64 = _TorchCpu(start, groups, torch.float32), _TorchCpu(start, groups, torch.float64)
    for s in range(5):
        g = _grads(shapes, s)
        f32.step(g, decays[s])
        f64.step(g, decays[s])
    clipped = [n.item() > 1 for n in f64.norms]
    assert any(clipped) and not all(clipped), f64.norms
    _parity(hip.tensors(), f32.tensors(), f64.tensors(), name)
    # the norm: exact squares, fp64 sums, one rounding -> within 1 fp32 ulp of the fp64 norm
    for got, ref in zip(hip.norms, f64.norms):
        ref32 = torch.tensor(ref.item(), dtype=torch.float32)
        ulp = (torch.nextafter(ref32, torch.tensor(math.inf)) - ref32).item()
        assert got.dtype == torch.float32 and got.ndim == 0 and got.is_cuda
        assert abs(got.double().item() - ref.item()) <= ulp, (got.item(), ref.item())
    # a second run from the same start: the same bits in every tensor
    again = run_hip()
    for n, ts in hip.tensors().items():
        for kind, a, b in zip(KINDS, ts, again.tensors()[n]):
            assert torch.equal(a, b), (n, kind)
    assert all(torch.equal(a, b) for a, b in zip(hip.norms, again.norms))


class _Odd(torch.nn.Module):
    """Sizes around the vector width and the chunk size, a parameter at a 4-byte-aligned address, and a buffer."""

    def __init__(self):
        super().__init__()
        gen = _gen(4)
        base = torch.randn(1001, generator=gen)
        self.a = torch.nn.Parameter(torch.randn(5, generator=gen))
        self.b = torch.nn.Parameter(torch.randn(8191, generator=gen))
        self.c = torch.nn.Parameter(torch.randn(3, 8193, generator=gen))
        self.d = torch.nn.Parameter(torch.randn(64, 64, generator=gen))
        self.e = torch.nn.Parameter(base[1:])
        self.register_buffer("running", torch.randn(7, generator=gen))


def _odd_pair():
    m = _Odd().to(DEV)
    m.e = torch.nn.Parameter(torch.randn(1001, generator=_gen(5)).to(DEV)[1:])       # .to() re-allocates: offset the address again
    assert m.e.data_ptr() % 16 == 4 and m.e.is_contiguous()
    avg = copy.deepcopy(m)
    avg.e = torch.nn.Parameter(m.e.detach().clone())
    with torch.no_grad():
        for p in avg.parameters():
            p.mul_(0.5)
        avg.running.zero_()
    return m, avg


def _set_grads(m, step):
    gen = _gen(70 + step)
    for p in m.parameters():
        g = torch.randn(p.shape, generator=gen).to(DEV)
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)


def _state(m, avg, opt):
    out = [p.detach().clone() for p in m.parameters()] + [p.detach().clone() for p in avg.parameters()]
    for p in m.parameters():
        out += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return out


def _odd_run(KD, **kw):
    m, avg = _odd_pair()
    opt = KD.optim.AdamW(m.parameters(), lr=1e-2, betas=BETAS)
    opt.attach_ema(m, avg)
    for s in range(3):
        _set_grads(m, s)
        kw_s = {k: (v[s] if isinstance(v, list) else v) for k, v in kw.items()}
        after = kw_s.pop("after", None)
        opt.step(**kw_s)
        if after:
            after(m, avg, s)
    return m, avg, opt


def test_step_options_against_the_unfused_composition(KD):
    decays = [0.0, 0.37, 0.9]
    # odd sizes and the unaligned tensor against torch itself (fp32 on the GPU; a few ulps of another operation order)
    m, avg, opt = _odd_run(KD, clip_grad_norm=1.0, ema_decay=decays)
    m2, avg2 = _odd_pair()
    ref = torch.optim.AdamW(m2.parameters(), lr=1e-2, betas=BETAS)
    for s in range(3):
        _set_grads(m2, s)
        torch.nn.utils.clip_grad_norm_(m2.parameters(), 1.0)
        ref.step()
        with torch.no_grad():
            for p, a in zip(m2.parameters(), avg2.parameters()):
                a.lerp_(p, 1 - decays[s])
    for (n, p), q, a, b in zip(m.named_parameters(), m2.parameters(), avg.parameters(), avg2.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), n
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), n
    # buffers are copied on a step with an EMA decay
    assert torch.equal(avg.running, m.running)
    base = _state(m, avg, opt)

    # zero_grad=True: the same update, gradients zero at unchanged addresses, version counters bumped
    seen = []

    def zeroed(m_, avg_, s):
        assert all(not p.grad.any() for p in m_.parameters())
        seen.append(([p.grad.data_ptr() for p in m_.parameters()], [p._version for p in m_.parameters()]))
    assert all(torch.equal(a, b) for a, b in zip(base, _state(*_odd_run(KD, clip_grad_norm=1.0, ema_decay=decays, zero_grad=True, after=zeroed))))
    assert seen[0][0] == seen[1][0] == seen[2][0] and all(b > a for a, b in zip(seen[0][1], seen[2][1]))

    # clip_grad_norm=None equals a step with a huge max_norm
    none = _state(*_odd_run(KD, ema_decay=decays))
    huge = _state(*_odd_run(KD, clip_grad_norm=1e30, ema_decay=decays))
    assert all(torch.equal(a, b) for a, b in zip(none, huge))
    assert not all(torch.equal(a, b) for a, b in zip(none, base))          # (and clipping at 1 did something)

    # ema_decay=None leaves the EMA model untouched
    _, avg0 = _odd_pair()
    mn, avgn, optn = _odd_run(KD, clip_grad_norm=1.0)
    assert all(torch.equal(a, b) for a, b in zip(avgn.parameters(), avg0.parameters())) and torch.equal(avgn.running, avg0.running)

    # ema_update stand-alone equals the fused EMA bit for bit
    alone = _state(*_odd_run(KD, clip_grad_norm=1.0, after=lambda m_, avg_, s: KD.utils.ema_update(m_, avg_, decays[s])))
    assert all(torch.equal(a, b) for a, b in zip(base, alone))

    # a parameter without a gradient is skipped by AdamW (as in torch) and still enters the average
    ms, avgs = _odd_pair()
    opts = KD.optim.AdamW(ms.parameters(), lr=1e-2, betas=BETAS)
    opts.attach_ema(ms, avgs)
    _set_grads(ms, 0)
    ms.d.grad = None
    before, avg_before = ms.d.detach().clone(), avgs.d.detach().clone()
    opts.step(ema_decay=0.37)
    assert torch.equal(ms.d, before) and len(opts.state[ms.d]) == 0
    assert torch.allclose(avgs.d, torch.lerp(avg_before, before, 1 - 0.37), rtol=1e-6, atol=1e-7) and not torch.equal(avgs.d, avg_before)
    # refusals: no fallback
    md = _Odd().to(DEV).double()
    optd = KD.optim.AdamW(md.parameters())
    for p in md.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(TypeError, match="float32"):
        optd.step()


def test_sigma_densities_against_the_reference(KD, monkeypatch):
    """The public ``rand_*`` functions with the draw replaced by the golden's recorded uniforms (and normals), as the golden script replaced
    the reference's: per density, the max relative error against the reference's fp64 output is at most 4 x the reference's own fp32 max
    relative error on the same case."""
    from safetensors.torch import load_file
    gold = json.load(open(os.path.join(cases.GOLDEN_DIR, "training.json")))["densities"]
    arrays = load_file(os.path.join(cases.GOLDEN_DIR, "training.safetensors"))
    u, normal = arrays["uniforms"], arrays["normals"]
    assert u[0] == 0 and u[1] == 1 - 2.0 ** -24 and len(u) >= 2000 and len(gold) >= 6
    monkeypatch.setattr(torch, "rand", lambda shape, device=None, dtype=None: u.to(device, dtype))
    monkeypatch.setattr(torch, "randn", lambda shape, device=None, dtype=None: normal.to(device, dtype))
    misses = {}
    for name, rec in gold.items():
        got = getattr(KD.utils, rec["func"])([len(u)], device=DEV, **rec["keywords"])
        assert got.dtype == torch.float32 and got.is_cuda
        got, ref32, ref64 = got.cpu().double(), arrays[name + ".fp32"].double(), arrays[name + ".fp64"]
        ok = torch.isfinite(ref64) & (ref64 != 0)
        assert ok.sum() >= len(u) - 4
        assert torch.equal(got[~ok], ref64[~ok].float().double()), name                 # exact zeros / infinities agree as such
        e_got = ((got[ok] - ref64[ok]).abs() / ref64[ok].abs()).max().item()
        e_ref = ((ref32[ok] - ref64[ok]).abs() / ref64[ok].abs()).max().item()
        print(f"density {name}: max rel err {e_got:.3e}, the reference's own fp32 {e_ref:.3e}")
        if not e_got <= 4 * e_ref:
            misses[name] = (e_got, e_ref)
    assert not misses, misses


def test_stratified_draws_and_public_densities(KD):
    U = KD.utils
    n, group, groups = 64, 1, 3
    lo, hi = 0.01, 80.0
    torch.manual_seed(3)
    with U.enable_stratified(group, groups):
        s = U.rand_log_uniform([4, n], lo, hi, device=DEV, dtype=torch.float64)
        s32 = U.rand_log_uniform([n], lo, hi, device=DEV)
    assert s.dtype == torch.float64 and s.shape == (4, n) and s.is_cuda and s32.dtype == torch.float32
    frac = (s.log() - math.log(lo)) / (math.log(hi) - math.log(lo))
    strata = torch.floor(frac * (n * groups)).long().cpu()
    assert torch.equal(strata, (group + torch.arange(n) * groups).expand(4, n)), strata
    frac32 = (s32.double().log() - math.log(lo)) / (math.log(hi) - math.log(lo)) * (n * groups)
    want = (group + torch.arange(n, device=DEV) * groups).double()
    assert ((frac32 > want - 1e-3) & (frac32 < want + 1 + 1e-3)).all()
    # outside the context manager (or disabled): plain uniforms, not one per stratum
    torch.manual_seed(3)
    plain = U.rand_log_uniform([n], lo, hi, device=DEV, dtype=torch.float64)
    frac = (plain.log() - math.log(lo)) / (math.log(hi) - math.log(lo))
    assert not torch.equal(torch.floor(frac * n).long().cpu(), torch.arange(n))
    with U.enable_stratified(0, 1, disable=True):
        assert U.stratified_with_settings([n], device=DEV).shape == (n,)
    su = U.stratified_uniform([n], 2, 4, dtype=torch.float64, device=DEV)
    assert torch.equal(torch.floor(su * 4 * n).long().cpu(), 2 + torch.arange(n) * 4)
    # the truncation bounds, dtype and device of the public functions
    torch.manual_seed(4)
    for dtype in (torch.float32, torch.float64):
        for fn, kw, a, b in [(U.rand_log_logistic, dict(loc=-0.7, scale=0.5, min_value=0.1, max_value=5.0), 0.1, 5.0),
                             (U.rand_v_diffusion, dict(sigma_data=0.5, min_value=0.02, max_value=30.0), 0.02, 30.0),
                             (U.rand_log_uniform, dict(min_value=0.3, max_value=0.4), 0.3, 0.4),
                             (U.rand_cosine_interpolated, dict(image_d=64, noise_d_low=32, noise_d_high=64, sigma_data=0.5, min_value=1e-3,
                                                               max_value=1e3), 1e-3, 1e3)]:
            x = fn([2000], device=DEV, dtype=dtype, **kw)
            assert x.dtype == dtype and x.is_cuda and x.shape == (2000,)
            assert x.min().item() >= a * (1 - 1e-6) and x.max().item() <= b * (1 + 1e-6), (fn.__name__, x.min().item(), x.max().item())
    x = U.rand_log_normal([20000], loc=-1.2, scale=1.2, device=DEV)
    assert abs(x.log().mean().item() + 1.2) < 0.05 and abs(x.log().std().item() - 1.2) < 0.05
    x = U.rand_split_log_normal([20000], loc=-1.0, scale_1=1.4, scale_2=0.9, device=DEV)
    left = (x.log() < -1.0).float().mean().item()
    assert abs(left - 1.4 / 2.3) < 0.03, left
    mc = {"sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80, "input_size": [32, 32], "sigma_sample_density": {"type": "cosine-interpolated"}}
    sigma = KD.training.make_sample_density(mc)([8], device=DEV)
    assert sigma.shape == (8,) and sigma.is_cuda and (sigma > 0).all()


def test_state_interchange_with_torch_adamw(KD):
    _, model = _model(KD, "tiny_sw")
    start = dict(model.named_parameters())
    groups = _group_names(model, LR)
    shapes = {n: p.shape for n, p in start.items()}
    names = list(start)
    hip = _Hip(KD, start, groups)
    for s in range(3):
        hip.step(_grads(shapes, s), None)
    sd = copy.deepcopy(hip.opt.state_dict())
    now = {n: p.detach().clone() for n, p in hip.p.items()}

    def torch_opt(params, device, dtype, state):
        ps = {n: torch.nn.Parameter(t.detach().to(device, dtype).clone()) for n, t in params.items()}
        opt = torch.optim.AdamW([{"params": [ps[n] for n in gnames], **kw} for gnames, kw in groups], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        opt.load_state_dict(copy.deepcopy(state))
        return ps, opt

    def torch_step(ps, opt, grads, device, dtype):
        for n, p in ps.items():
            p.grad = grads[n].to(device, dtype)
        torch.nn.utils.clip_grad_norm_(list(ps.values()), 1.0)
        opt.step()

    def triple(ps, opt):
        return {n: (ps[n].detach(), opt.state[ps[n]]["exp_avg"], opt.state[ps[n]]["exp_avg_sq"]) for n in names}

    def compare(fused, tp, topt, dp, dopt, what):
        h = fused.tensors()
        _parity({n: h[n][:3] for n in names}, {n: tuple(t.cpu() for t in triple(tp, topt)[n]) for n in names}, triple(dp, dopt), what)

    # fused state -> torch.optim.AdamW: a fourth step on both, and in fp64 from the same state
    g3 = _grads(shapes, 2)                      # (a clipped step)
    tp, topt = torch_opt(now, DEV, torch.float32, sd)
    dp, dopt = torch_opt(now, "cpu", torch.float64, sd)
    assert all(int(topt.state[p]["step"]) == 3 for p in tp.values())
    torch_step(tp, topt, g3, DEV, torch.float32)
    torch_step(dp, dopt, g3, "cpu", torch.float64)
    hip.step(g3, None)
    compare(hip, tp, topt, dp, dopt, "fused -> torch, step 4")
    # torch state -> the fused optimizer: a fifth step on both
    sd4 = copy.deepcopy(topt.state_dict())
    now4 = {n: p.detach().clone() for n, p in tp.items()}
    back = _Hip(KD, now4, groups)
    back.opt.load_state_dict(copy.deepcopy(sd4))
    dp, dopt = torch_opt(now4, "cpu", torch.float64, sd4)
    g4 = _grads(shapes, 4)
    torch_step(tp, topt, g4, DEV, torch.float32)
    torch_step(dp, dopt, g4, "cpu", torch.float64)
    back.step(g4, None)
    assert all(int(back.opt.state[p]["step"]) == 5 for p in back.p.values())
    compare(back, tp, topt, dp, dopt, "torch -> fused, step 5")


def test_plan_follows_the_fused_updates(KD):
    """test_train_then_sample of tests/test_param_grad_gpu.py on the fused optimizer: the step writes the parameters through raw pointers,
    so the launch plan and the packed weight images follow only if the step bumps the version counters."""
    cfg, model = _model(KD, "tiny_sw")
    mc = cfg["model"]
    model = model.to(DEV).eval()
    model_ema = copy.deepcopy(model)
    gen = _gen(41)
    x = (torch.randn(4, mc["input_channels"], *mc["input_size"], generator=gen) * 0.5).to(DEV)
    noise = torch.randn(x.shape, generator=gen).to(DEV)
    sigma = torch.tensor([0.3, 6.0, 1.1, 25.0], device=DEV)
    kw = {"class_cond": ((torch.arange(4) * 3 + 1) % 11).to(DEV)}
    den, den_ema = KD.Denoiser(model, mc["sigma_data"]), KD.Denoiser(model_ema, mc["sigma_data"])
    opt = KD.optim.AdamW(model.param_groups(2e-3), betas=(0.9, 0.99))
    opt.attach_ema(model, model_ema)
    with torch.no_grad():                           # forwards through the launch plans before training
        den(x, sigma, **kw)
        den_ema(x, sigma, **kw)
    losses = []
    for _ in range(6):
        loss = den.loss(x, noise, sigma, **kw).mean()
        loss.backward()
        opt.step(clip_grad_norm=10.0, ema_decay=0.5, zero_grad=True)
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    for trained, wrapper in ((model, den), (model_ema, den_ema)):
        fresh = KD.config.make_model(cfg).eval()
        fresh.load_state_dict({k: v.cpu() for k, v in trained.state_dict().items()})
        fresh = fresh.to(DEV)
        with torch.no_grad():
            a = wrapper(x, sigma, **kw)
            b = KD.Denoiser(fresh, mc["sigma_data"])(x, sigma, **kw)
        assert torch.equal(a, b)
    with torch.no_grad():
        assert not torch.equal(den(x, sigma, **kw), den_ema(x, sigma, **kw))


def _run_train(cwd, args, timeout=420):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


def test_train_py_end_to_end(KD, tmp_path):
    from PIL import Image
    data_dir = tmp_path / "images"
    data_dir.mkdir()
    gen = _gen(8)
    for i in range(16):
        arr = (torch.rand(16, 16, 3, generator=gen) * 255).to(torch.uint8).numpy()
        Image.fromarray(arr, mode="RGB").save(data_dir / f"img_{i:02}.png")
    config = {"model": {"type": "image_transformer_v2", "input_channels": 3, "input_size": [16, 16], "patch_size": [2, 2], "depths": [1, 1],
                        "widths": [64, 128], "self_attns": [{"type": "shifted-window", "d_head": 64, "window_size": 4},
                                                            {"type": "global", "d_head": 64}],
                        "loss_config": "karras", "loss_weighting": "soft-min-snr", "dropout_rate": [0.0, 0.0], "augment_prob": 0.0,
                        "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80, "sigma_sample_density": {"type": "cosine-interpolated"}},
              "dataset": {"type": "imagefolder", "location": str(data_dir)},
              "optimizer": {"type": "adamw", "lr": 5e-4, "betas": [0.9, 0.95], "eps": 1e-8, "weight_decay": 1e-3},
              "lr_sched": {"type": "constant", "warmup": 0.0}, "ema_sched": {"type": "inverse", "power": 0.75, "max_value": 0.9999}}
    (tmp_path / "config.json").write_text(json.dumps(config))
    common = ["--config", str(tmp_path / "config.json"), "--batch-size", "4", "--grad-accum-steps", "2", "--save-every", "3", "--demo-every", "6",
              "--sample-n", "4", "--seed", "1", "--num-workers", "0"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _run_train(a, [*common, "--end-step", "6", "--name", "run"])
    for f in ("run_00000003.pth", "run_00000006.pth", "run_state.json", "run_log.csv", "run_demo_00000006.png"):
        assert (a / f).exists(), f
    assert json.load(open(a / "run_state.json")) == {"latest_checkpoint": "run_00000006.pth"}
    assert len((a / "run_log.csv").read_text().strip().splitlines()) == 7
    assert Image.open(a / "run_demo_00000006.png").size == (32, 32)
    full = torch.load(a / "run_00000006.pth", map_location="cpu", weights_only=False)
    assert {"model", "model_ema", "opt", "sched", "ema_sched", "epoch", "step", "gns_stats", "ema_stats"} <= set(full)
    assert full["step"] == 6 and full["gns_stats"] is None and full["ema_sched"]["last_epoch"] == 3
    _run_train(b, [*common, "--end-step", "6", "--name", "run", "--resume", str(a / "run_00000003.pth")])
    resumed = torch.load(b / "run_00000006.pth", map_location="cpu", weights_only=False)
    for key in ("model", "model_ema"):
        assert full[key].keys() == resumed[key].keys()
        assert all(torch.equal(full[key][k], resumed[key][k]) for k in full[key]), key
    assert not all(torch.equal(full["model"][k], full["model_ema"][k]) for k in full["model"])
    assert full["opt"]["state"].keys() == resumed["opt"]["state"].keys() and len(full["opt"]["state"]) > 0
    for i, st in full["opt"]["state"].items():
        assert all(torch.equal(st[k], resumed["opt"]["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq")), i
    assert full["opt"]["param_groups"] == resumed["opt"]["param_groups"]

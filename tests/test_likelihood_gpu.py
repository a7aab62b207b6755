"""log_likelihood on the MI355X: the tangent kernels of csrc/jvp_f32.hip against the CPU oracle's functions differentiated in fp64, the
dual pass of the model against the oracle forward under a JVP, the ODE function against the reference (tests/golden/ll_odefn.safetensors,
recorded by tests/golden/make_golden_ll.py), and whole log_likelihood runs (a Gaussian with a known answer, an fp64 CPU dopri5 over the
oracle, determinism, the refusals)."""
import math

import pytest
import torch
from torch.autograd.functional import jvp as fd_jvp

from oracle import hdit
from tests.golden import cases
from tests.golden import make_golden_ll as mgl
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
KTOL = 1e-5           # kernels vs fp64: fp32 rounding


def g(t):
    return t.to(DEV, torch.float32).contiguous()


def d64(*ts):
    return [t.double() for t in ts]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("rows,d,B", [(64, 128, 2), (50, 256, 5), (7, 512, 1)])
def test_rmsnorm_jvp(KD, rows, d, B):
    gen = _gen(rows + d)
    x, xd = torch.randn(B, rows, d, generator=gen), torch.randn(B, rows, d, generator=gen)
    ada = torch.rand(B, 1, d, generator=gen) + 0.5
    gain = torch.rand(d, generator=gen) + 0.5
    for scale, arg in ((ada, ada[:, 0]), (gain, gain)):
        y_ref, yd_ref = fd_jvp(lambda t: hdit.rms_norm(t, scale.double()), x.double(), xd.double())
        y, yd = KD.ops.rms_norm_jvp(g(x), g(xd), g(arg), rows_per_sample=rows)
        assert relerr(y, y_ref) < KTOL and relerr(yd, yd_ref) < KTOL


def test_geglu_jvp(KD):
    gen = _gen(3)
    h, hd = torch.randn(3, 37, 2 * 96, generator=gen) * 3, torch.randn(3, 37, 2 * 96, generator=gen)
    f = lambda t: t[..., :96] * torch.nn.functional.gelu(t[..., 96:])
    y_ref, yd_ref = fd_jvp(f, h.double(), hd.double())
    y, yd = KD.ops.geglu_jvp(g(h), g(hd))
    assert relerr(y, y_ref) < KTOL and relerr(yd, yd_ref) < KTOL


def _pack(q, k, v):
    return torch.stack([q, k, v], dim=3).reshape(*q.shape[:3], -1).contiguous()


def _tables(h, w, nh):
    theta = hdit.rope_theta(hdit.axial_pos(h, w), hdit.rope_freqs(nh)).reshape(h * w, nh, 16)
    return torch.cos(theta), torch.sin(theta)


@pytest.mark.parametrize("B,H,W,nh", [(2, 8, 8, 2), (3, 5, 7, 4)])
def test_qk_prep_jvp(KD, B, H, W, nh):
    gen = _gen(H * W + nh)
    qkv, qkvd = torch.randn(B, H, W, 3 * nh * 64, generator=gen), torch.randn(B, H, W, 3 * nh * 64, generator=gen)
    scale = torch.linspace(4.0, 12.0, nh)

    def f(t):
        q, k, v = hdit.split_qkv(t, nh)
        q, k = hdit.cosine_sim_scale(q, k, scale.double())
        theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
        return _pack(hdit.apply_rope(q, theta), hdit.apply_rope(k, theta), v)
    y_ref, yd_ref = fd_jvp(f, qkv.double(), qkvd.double())
    cos, sin = _tables(H, W, nh)
    a, ad = g(qkv), g(qkvd)
    KD.ops.qk_prep_jvp_(a, ad, g(scale), g(cos), g(sin), nh)
    assert relerr(a, y_ref) < KTOL and relerr(ad, yd_ref) < KTOL


def _attn_case(B, H, W, nh, seed, fn, call):
    """Prepared q, k (unit rows times sqrt(10), like the cosine-sim scale) and v; the oracle ``fn`` under a JVP in fp64 vs ``call``."""
    gen = _gen(seed)
    q, k, v = (torch.randn(B, H, W, nh, 64, generator=gen) for _ in range(3))
    q, k = hdit.cosine_sim_scale(q, k, torch.full([nh], 10.0))
    qd, kd, vd = (torch.randn(B, H, W, nh, 64, generator=gen) * 0.3 for _ in range(3))
    qkv, qkvd = _pack(q, k, v), _pack(qd, kd, vd)

    def f(t):
        a, b, c = hdit.split_qkv(t, nh)
        return fn(a, b, c).reshape(B, H, W, nh * 64)
    o_ref, od_ref = fd_jvp(f, qkv.double(), qkvd.double())
    o, od = call(g(qkv), g(qkvd))
    torch.cuda.synchronize()
    assert relerr(o, o_ref) < KTOL, relerr(o, o_ref)
    assert relerr(od, od_ref) < KTOL, relerr(od, od_ref)
    o2, od2 = call(g(qkv), g(qkvd))
    assert torch.equal(o, o2) and torch.equal(od, od2)            # deterministic


@pytest.mark.parametrize("B,H,W,nh", [(2, 7, 7, 2), (1, 16, 16, 2), (2, 5, 7, 3), (1, 1, 3, 1)])
def test_attn_global_jvp(KD, B, H, W, nh):
    _attn_case(B, H, W, nh, 10 + H * W, hdit.attn_global, lambda a, b: KD.ops.attn_global_jvp(a, b, nh))


@pytest.mark.parametrize("ks", [3, 5, 7, 9, 11, 13])
@pytest.mark.parametrize("H,W", [(13, 17), (16, 16)])
def test_attn_na2d_jvp(KD, ks, H, W):
    _attn_case(2, H, W, 2, ks * 100 + H, lambda a, b, c: hdit.na2d(a, b, c, ks), lambda a, b: KD.ops.attn_na2d_jvp(a, b, 2, ks))


@pytest.mark.parametrize("ws,H,W", [(4, 8, 12), (8, 16, 8), (8, 16, 16), (16, 16, 32)])
@pytest.mark.parametrize("half", [False, True])
def test_attn_window_jvp(KD, ws, H, W, half):
    shift = ws // 2 if half else 0
    _attn_case(2, H, W, 2, ws * 10 + H + half, lambda a, b, c: hdit.attn_shifted_window(a, b, c, ws, shift),
               lambda a, b: KD.ops.attn_window_jvp(a, b, 2, ws, shift))


def test_ll_div_and_prior(KD):
    gen = _gen(5)
    x, D, Dd = (torch.randn(3, 2, 9, 11, generator=gen) for _ in range(3))
    v = torch.randint(0, 2, x.shape, generator=gen).float() * 2 - 1
    sigma = torch.tensor([0.1, 2.0, 70.0])
    d, d_ll = KD.ops.ll_div(g(x), g(D), g(Dd), g(v), g(sigma))
    x64, D64, Dd64, v64 = d64(x, D, Dd, v)
    assert relerr(d, (x64 - D64) / sigma.double().view(-1, 1, 1, 1)) < KTOL
    assert relerr(d_ll, (v64 * (v64 - Dd64)).flatten(1).sum(1) / sigma.double()) < KTOL
    lp = KD.ops.gauss_logp(g(x), 3.5, add=g(sigma))
    ref = torch.distributions.Normal(0.0, 3.5).log_prob(x.double()).flatten(1).sum(1) + sigma.double()
    assert relerr(lp, ref) < KTOL


def test_rk_combine_and_error(KD):
    gen = _gen(6)
    ks = [torch.randn(1000, generator=gen) for _ in range(7)]
    y0, y1 = torch.randn(1000, generator=gen), torch.randn(1000, generator=gen)
    c = [0.3, -1.2, 0.0, 2.5, 0.1, -0.7, 1.0 / 60]
    out = KD.ops.rk_combine(g(y0), [g(k) for k in ks], c)
    ref = y0.double() + sum(ci * k.double() for ci, k in zip(c, ks))
    assert relerr(out, ref) < KTOL
    e = KD.ops.rk_error_sq([g(k) for k in ks], c, g(y0), g(y1), 1e-4, 1e-3)
    err = sum(ci * k.double() for ci, k in zip(c, ks)) / (1e-4 + 1e-3 * torch.maximum(y0.abs(), y1.abs()).double())
    assert abs(e - float(err.pow(2).sum())) < 1e-5 * float(err.pow(2).sum())
    assert KD.ops.rk_error_sq([g(k) for k in ks], c, g(y0), g(y1), 1e-4, 1e-3) == e


# ---------------------------------------------------------------------------------------------------------- the dual pass

_models = {}


def build(KD, name):
    if name not in _models:
        cfg = KD.config.load_config(cases.raw_config(name))
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        sd = KD.synth.synth_state_dict(model.state_dict(), seed=cases.WEIGHT_SEED)
        model.load_state_dict(sd)
        _models[name] = (cfg, model.to(DEV), sd)
    return _models[name]


def _oracle_denoiser(cfg, sd, cls):
    mc = cfg["model"]
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def den(x, sigma):
        torch.set_default_dtype(torch.float64)
        try:
            sdata = mc["sigma_data"]
            var = sigma ** 2 + sdata ** 2
            c_skip, c_out, c_in = (sdata ** 2 / var).view(-1, 1, 1, 1), (sigma * sdata / var ** 0.5).view(-1, 1, 1, 1), (1 / var ** 0.5).view(-1, 1, 1, 1)
            return hdit.forward(sd64, mc, x * c_in, sigma, class_cond=cls) * c_out + x * c_skip
        finally:
            torch.set_default_dtype(torch.float32)
    return den


@pytest.mark.parametrize("name,batch", [("tiny_global", 2), ("tiny_sw", 2), ("tiny_na", 2), ("tiny_odd", 2), ("mnist", 1), ("cifar", 1)])
@pytest.mark.parametrize("mode,ttol", [("exact", 1e-4), ("split3", 3e-4)])
def test_denoiser_forward_jvp(KD, monkeypatch, name, batch, mode, ttol):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    cfg, model, sd = build(KD, name)
    mc = cfg["model"]
    gen = _gen(31)
    sigma = torch.tensor([0.4, 7.0][:batch])
    x = torch.randn(batch, mc["input_channels"], *mc["input_size"], generator=gen) * (sigma.view(-1, 1, 1, 1) ** 2 + 0.25).sqrt()
    v = torch.randint(0, 2, x.shape, generator=gen).float() * 2 - 1
    nc = cases.num_classes_of(cfg)
    cls = (torch.arange(batch) * 3 + 1) % (nc + 1) if nc else None
    kw = {"class_cond": cls.to(DEV)} if cls is not None else {}
    den = KD.Denoiser(model, mc["sigma_data"])
    out, out_d = den.forward_jvp(g(x), g(sigma), g(v), **kw)
    prim = den(g(x), g(sigma), **kw)
    assert relerr(out, prim) < 5e-4, relerr(out, prim)
    ref, ref_d = fd_jvp(lambda t: _oracle_denoiser(cfg, sd, cls)(t, sigma.double()), x.double(), v.double())
    assert relerr(out, ref) < ttol, relerr(out, ref)
    assert relerr(out_d, ref_d) < ttol, relerr(out_d, ref_d)
    out2, out_d2 = den.forward_jvp(g(x), g(sigma), g(v), **kw)
    assert torch.equal(out, out2) and torch.equal(out_d, out_d2)


def test_forward_jvp_leaves_the_plan_cache_alone(KD):
    cfg, model, _ = build(KD, "tiny_sw")
    x = torch.randn(3, 3, 32, 32, device=DEV)
    before = dict(model._plans)
    KD.Denoiser(model, 0.5).forward_jvp(x, torch.full((3,), 1.0, device=DEV), torch.ones_like(x), class_cond=torch.tensor([1, 2, 3], device=DEV))
    assert model._plans.keys() == before.keys() and all(model._plans[k] is before[k] for k in before)


def test_ode_function_vs_reference(KD, monkeypatch):
    """(d, d_ll) of the HIP path at the golden's points and probe against the reference's own closure (autograd through its model)."""
    from safetensors.torch import load_file
    import os
    monkeypatch.setenv("KDIFF_GEMM", "exact")
    gold = load_file(os.path.join(cases.GOLDEN_DIR, "ll_odefn.safetensors"))
    for name, batch in mgl.LL_CASES:
        cfg, model, _ = build(KD, name)
        xs, cls = mgl.ll_points(cfg, batch)
        kw = {"class_cond": cls.to(DEV)} if cls is not None else {}
        den = KD.Denoiser(model, cfg["model"]["sigma_data"])
        v = g(gold[f"{name}.v"])
        for i, s in enumerate(mgl.LL_SIGMAS):
            x = g(xs[i])
            sig = torch.full((batch,), s, device=DEV)
            D, Dd = den.forward_jvp(x, sig, v, **kw)
            d, d_ll = KD.ops.ll_div(x, D, Dd, v, sig)
            assert relerr(d, gold[f"{name}.{i}.d"]) < 2e-4, (name, s, relerr(d, gold[f"{name}.{i}.d"]))
            assert relerr(d_ll, gold[f"{name}.{i}.d_ll"]) < 2e-4, (name, s, d_ll.tolist(), gold[f"{name}.{i}.d_ll"].tolist())


# ---------------------------------------------------------------------------------------------------------- log_likelihood

def test_gaussian_known_answer(KD):
    """Data ~ N(0, s^2 I) has the denoiser D(x, sigma) = x s^2 / (s^2 + sigma^2) and log p_{sigma_min}(x) = sum log N(x; 0, s^2 + sigma_min^2);
    the model is a plain torch function, so the reference's autograd formulation runs (the solver arithmetic is HIP)."""
    s, smin, smax = 0.5, 1e-2, 80.0
    torch.manual_seed(3)
    x = (torch.randn(2, 3, 8, 8) * math.sqrt(s * s + smin * smin)).to(DEV)

    def model(xx, sigma):
        return xx * (s * s / (s * s + sigma ** 2)).view(-1, 1, 1, 1)
    ll, info = KD.likelihood.log_likelihood(model, x, smin, smax)
    ref = torch.distributions.Normal(0.0, math.sqrt(s * s + smin * smin)).log_prob(x.double().cpu()).flatten(1).sum(1)
    assert relerr(ll, ref) < 1e-3, (ll.tolist(), ref.tolist())
    assert info["fevals"] >= 8 and (info["fevals"] - 2) % 6 == 0


class _CpuVec:
    @staticmethod
    def combine(y0, ks, coeffs):
        return tuple(y + sum(c * k[n] for k, c in zip(ks, coeffs)) for n, y in enumerate(y0))

    @staticmethod
    def norm(ks, coeffs, y0, y1, atol, rtol):
        out = 0.0
        for n, y in enumerate(y0):
            err = sum(c * k[n] for k, c in zip(ks, coeffs))
            ref = y.abs() if y1 is None else torch.maximum(y.abs(), y1[n].abs())
            out = max(out, float((err / (atol + rtol * ref)).pow(2).mean().sqrt()))
        return out


def test_tiny_global_vs_fp64_cpu_solver(KD, monkeypatch):
    """The HIP path against the same dopri5 rules run in fp64 on the CPU over the oracle under autograd (the reference's formulation).
    Gate: ll to 1e-3 relative (the two runs take their own step sequences; the ODE itself is solved to rtol = atol = 1e-4), fevals within
    one step (6 evaluations)."""
    monkeypatch.setenv("KDIFF_GEMM", "exact")
    cfg, model, sd = build(KD, "tiny_global")
    mc = cfg["model"]
    torch.manual_seed(0)
    x = torch.randn(2, 3, 16, 16) * 0.5
    den = KD.Denoiser(model, mc["sigma_data"])
    torch.manual_seed(11)
    ll, info = KD.likelihood.log_likelihood(den, x.to(DEV), mc["sigma_min"], mc["sigma_max"])
    torch.manual_seed(11)
    v = (torch.randint_like(x.to(DEV), 2) * 2 - 1).cpu().double()
    oden = _oracle_denoiser(cfg, sd, None)
    fevals = 0

    def f(t, y):
        nonlocal fevals
        fevals += 1
        sig = torch.full((2,), t, dtype=torch.float64)
        with torch.enable_grad():
            xx = y[0].detach().requires_grad_()
            d = (xx - oden(xx, sig)) / t
            grad = torch.autograd.grad((d * v).sum(), xx)[0]
        return d.detach(), (v * grad).flatten(1).sum(1)
    lat, dll = KD.likelihood.dopri5(f, (x.double(), torch.zeros(2, dtype=torch.float64)), mc["sigma_min"], mc["sigma_max"], 1e-4, 1e-4,
                                    vec=_CpuVec)
    ref = torch.distributions.Normal(0.0, float(mc["sigma_max"])).log_prob(lat).flatten(1).sum(1) + dll
    print(f"tiny_global: HIP ll {ll.tolist()} fevals {info['fevals']}; fp64 CPU ll {ref.tolist()} fevals {fevals}")
    assert relerr(ll, ref) < 1e-3, (ll.tolist(), ref.tolist())
    assert abs(info["fevals"] - fevals) <= 6


def test_seeded_runs_are_identical(KD):
    cfg, model, _ = build(KD, "tiny_sw")
    mc = cfg["model"]
    x = torch.randn(2, 3, 32, 32, generator=_gen(2)).to(DEV) * 0.5
    den = KD.Denoiser(model, mc["sigma_data"])
    kw = {"class_cond": torch.tensor([1, 10], device=DEV)}
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        runs.append(KD.likelihood.log_likelihood(den, x, mc["sigma_min"], mc["sigma_max"], extra_args=kw))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert torch.isfinite(runs[0][0]).all()


def test_refusals(KD):
    cfg, model, _ = build(KD, "tiny_global")
    den = KD.Denoiser(model, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.likelihood.log_likelihood(den, torch.randn(1, 3, 16, 16), 0.01, 80)
    vden = KD.external.VDenoiser(model)
    with pytest.raises(NotImplementedError, match="forward_jvp rule") as e:
        KD.likelihood.log_likelihood(vden, torch.randn(1, 3, 16, 16, device=DEV), 0.01, 80)
    assert "does not require grad" not in str(e.value)
    cfg_fn = KD.sampling.make_cfg_model_fn(den, 2.0, 10)
    with pytest.raises(NotImplementedError, match="forward_jvp rule"):
        KD.likelihood.log_likelihood(cfg_fn, torch.randn(1, 3, 16, 16, device=DEV), 0.01, 80, extra_args={"class_cond": torch.tensor([1], device=DEV)})

    class Foreign(torch.nn.Module):
        def forward(self, x, sigma):
            return x
    with pytest.raises(NotImplementedError, match="forward_jvp rule"):
        KD.likelihood.log_likelihood(KD.Denoiser(Foreign(), 0.5), torch.randn(1, 3, 16, 16, device=DEV), 0.01, 80)

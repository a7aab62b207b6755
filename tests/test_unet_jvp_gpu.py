"""The dual (forward-mode JVP) pass of the image_v1 U-Net on the MI355X: the AdaGN dual kernels and the stacked convolution (csrc/unet_f32.hip,
csrc/conv_x3.hip), ``forward_jvp`` of the model and of ``Denoiser`` around it, and ``log_likelihood`` end to end.  Truth is fp64 on the CPU:
``torch.func.jvp`` of the restatement (tests/test_unet_jvp_cpu.py: ``forward_fn`` / ``denoiser_fn``) and of ``adagn_expr``.

Bounds.
* AdaGN dual, y and y_dot: the rule of tests/test_unet_gpu.py -- ``base`` = the error of the SAME ``torch.func.jvp`` in fp32 on the CPU against
  fp64; the kernel is allowed 4 x base.  ``stats`` and y are the forward kernels' bits.
* jstats (from the formats): fp64 sums over <= 8192 elements, x centred with the fp64 mean, one fp32 rounding of the result: 2^-23 of the largest.
* stacked conv: bit for bit the existing entry's output per half (same kernel, the accumulation order of an output does not depend on the batch).
* model: the primal is the forward's bits; the tangent is within 5e-4 (max-abs relative, the forward's own gate) of the fp64 JVP, for F and for D.
* log_likelihood: the gates of tests/test_likelihood_gpu.py::test_tiny_global_vs_fp64_cpu_solver (ll to 1e-3 relative, fevals within 6).
"""
import ctypes as C
import functools

import pytest
import torch

from tests import unet_ref as ur
from tests.guard import Case, run_case
from tests.helpers import relerr
from tests.test_likelihood_gpu import _CpuVec
from tests.test_unet_gpu import (DEV, F32, SPLIT3, _kw, _lib_call, _p, adagn_expr, adagn_reference, built, conv_reference, g, nchw, rel, rn, tokens,
                                 within)
from tests.test_unet_jvp_cpu import denoiser_fn, forward_fn

pytestmark = pytest.mark.gpu


# ---- 1. AdaGN dual ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def adagn_jvp_reference(chan, hw, shifted, gelu):
    """(x, x_dot, w, b, y64, yd64, base_y, base_yd): the fp64 JVP of ``adagn_expr`` along x_dot and the fp32 JVP's own error, computed once."""
    B, (H, W) = 3, hw
    x, w, b, _, _ = adagn_reference(chan, hw, shifted, gelu)
    xd = rn(B, chan, H, W, seed=chan + 3 * H + (50 if shifted else 0) + 7)
    y64, yd64 = torch.func.jvp(lambda t: adagn_expr(t, w.double(), b.double(), chan // 32, gelu), (x.double(),), (xd.double(),))
    y32, yd32 = torch.func.jvp(lambda t: adagn_expr(t, w, b, chan // 32, gelu), (x,), (xd,))
    return x, xd, w, b, y64, yd64, (y32.double() - y64).abs().max().item(), (yd32.double() - yd64).abs().max().item()


def jstats_reference(xt, xdt, B, groups, eps=1e-5):
    """[B, groups, 4] = (mean_dot, rstd_dot, 0, 0) of fp64 tokens [B hw, C]."""
    chan = xt.shape[1]
    xg = xt.reshape(B, -1, groups, chan // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)
    dg = xdt.reshape(B, -1, groups, chan // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)
    mean, var = xg.mean(-1, keepdim=True), xg.var(-1, unbiased=False)
    rstd_dot = -(var + eps) ** -1.5 * ((xg - mean) * dg).mean(-1)
    return torch.stack([dg.mean(-1), rstd_dot, torch.zeros_like(rstd_dot), torch.zeros_like(rstd_dot)], dim=-1)


@pytest.mark.parametrize("chan,hw,shifted,gelu,layout", [(64, (7, 7), False, True, "plain"), (128, (16, 16), False, False, "wide"),
                                                         (64, (16, 16), True, True, "inplace"), (128, (7, 7), True, False, "plain"),
                                                         (64, (2, 2), False, True, "plain")], ids=str)
def test_adagn_jvp_matches_fp64(KD, chan, hw, shifted, gelu, layout):
    uo = KD.unet_ops
    B, (H, W), groups = 3, hw, chan // 32
    x, xd, w, b, y64, yd64, base_y, base_yd = adagn_jvp_reference(chan, hw, shifted, gelu)
    rows = B * H * W
    xt, xdt, wb = g(tokens(x)), g(tokens(xd)), g(torch.cat([w, b], dim=1))
    want_stats = uo.groupnorm_stats(xt, B, groups)
    want_y = uo.adagn_apply(xt, want_stats, wb, gelu=gelu)
    fills = []
    if layout == "wide":        # inputs: the right halves of NaN-filled [rows, 2 C] buffers; outputs: the left halves of buffers whose right halves stay
        xin, din = (torch.full((rows, 2 * chan), float("nan"), device=DEV) for _ in range(2))
        xin[:, chan:], din[:, chan:] = xt, xdt
        xin, din = xin[:, chan:], din[:, chan:]
        fills = [torch.full((rows, 2 * chan), -7.0, device=DEV) for _ in range(2)]
        out, out_dot = fills[0][:, :chan], fills[1][:, :chan]
    elif layout == "inplace":
        xin, din = xt.clone(), xdt.clone()
        out, out_dot = xin, din
    else:
        xin, din, out, out_dot = xt, xdt, None, None
    stats, jstats = uo.groupnorm_stats_jvp(xin, din, B, groups)
    again = uo.groupnorm_stats_jvp(xin, din, B, groups)
    y, yd = uo.adagn_apply_jvp(xin, din, stats, jstats, wb, gelu=gelu, out=out, out_dot=out_dot)
    what = f"adagn jvp C{chan} {H}x{W} shifted={shifted} gelu={gelu} {layout}"
    assert torch.equal(stats, want_stats), "the dual statistics are not groupnorm_stats's bits"
    assert torch.equal(again[0], stats) and torch.equal(again[1], jstats)
    js64 = jstats_reference(tokens(x).double(), tokens(xd).double(), B, groups)
    e_js = (jstats.cpu().double() - js64).abs().max().item() / js64.abs().max().item()
    print(f"{what}: jstats {e_js:.3e} of the largest ({2.0 ** -23:.3e})")
    assert e_js < 2.0 ** -23
    within(nchw(y, B, H, W), y64, base_y, what + " y")
    within(nchw(yd, B, H, W), yd64, base_yd, what + " y_dot")
    assert torch.equal(y, want_y), "the dual pass's primal is not adagn_apply's bits"
    for buf in fills:
        assert bool((buf[:, chan:] == -7.0).all()), "the columns beside the output range were written"
    if layout == "inplace":
        assert y.data_ptr() == xin.data_ptr() and yd.data_ptr() == din.data_ptr()
        xin, din = xt.clone(), xdt.clone()
        y2, yd2 = uo.adagn_apply_jvp(xin, din, stats, jstats, wb, gelu=gelu, out=xin, out_dot=din)
    else:
        y2, yd2 = uo.adagn_apply_jvp(xin, din, stats, jstats, wb, gelu=gelu)
    assert torch.equal(y2, y) and torch.equal(yd2, yd), "a repeat gives other bits"


def test_adagn_jvp_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    x = g(rn(2 * 4, 64))
    with pytest.raises(ValueError, match="tangent shape"):
        uo.groupnorm_stats_jvp(x, x[:4], 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.groupnorm_stats_jvp(x, x.cpu(), 2, 2)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        uo.groupnorm_stats_jvp(x, x.clone(), 2, 32)
    stats, jstats = uo.groupnorm_stats_jvp(x, x.clone(), 2, 2)
    with pytest.raises(RuntimeError, match="not crossed"):
        uo.adagn_apply_jvp(x, x.clone(), stats, jstats, g(rn(2, 128)), out_dot=x)


# ---- 2. stacked convolution ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ks,ci,co,hw,bias,residual,wide", [(3, 64, 128, (7, 7), True, False, False), (1, 128, 384, (5, 9), True, True, True),
                                                            (3, 128, 128, (5, 9), False, False, False)], ids=lambda v: str(v).replace(" ", ""))
def test_stacked_conv_is_the_plain_conv_per_half(KD, ks, ci, co, hw, bias, residual, wide):
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    x, w, b, r, _, _ = conv_reference(ks, ci, co, hw, bias, residual)
    seed = 100 * ks + ci + co + 7 * H + W
    xd = rn(B, ci, H, W, seed=seed + 11) * torch.logspace(-3, 3, ci)[None, :, None, None]
    rd = rn(B, co, H, W, seed=seed + 12) if residual else None
    rows = B * H * W
    xs = g(torch.cat([tokens(x), tokens(xd)]))
    rs = g(torch.cat([tokens(r), tokens(rd)])) if residual else None
    wt, bt = g(w), None if b is None else g(b)
    ybuf = torch.full((2 * rows, co + 64), -7.0, device=DEV) if wide else None
    y = uo.conv2d(xs, wt, 2 * B, H, W, bias=bt, residual=rs, out=ybuf[:, :co] if wide else None, bias_batch=B)
    primal = uo.conv2d(xs[:rows], wt, B, H, W, bias=bt, residual=None if rs is None else rs[:rows])
    tangent = uo.conv2d(xs[rows:], wt, B, H, W, bias=None, residual=None if rs is None else rs[rows:])
    assert torch.equal(y[:rows], primal), "the primal half is not kd_conv2d_x3's output"
    assert torch.equal(y[rows:], tangent), "the tangent half is not kd_conv2d_x3's output without the bias"
    if bias:
        assert not torch.equal(tangent, uo.conv2d(xs[rows:], wt, B, H, W, bias=bt, residual=None if rs is None else rs[rows:]))
    if wide:
        assert bool((ybuf[:, co:] == -7.0).all()), "the columns beside the output range were written"
    # bias_batch = batch is the plain entry; bias_batch outside 0 .. batch is refused
    assert torch.equal(uo.conv2d(xs[:rows], wt, B, H, W, bias=bt, bias_batch=B), uo.conv2d(xs[:rows], wt, B, H, W, bias=bt))
    with pytest.raises(RuntimeError, match="bias_batch"):
        uo.conv2d(xs[:rows], wt, B, H, W, bias=bt, bias_batch=B + 1)


# ---- 3. guard bands: one ragged shape per new entry point ---------------------------------------------------------------------------------------

def _stats_jvp_case():
    def make(env):
        chan, hw = 64, (7, 7)
        x, xd, *_ = adagn_jvp_reference(chan, hw, False, True)
        B, groups = x.shape[0], chan // 32
        js64 = jstats_reference(tokens(x).double(), tokens(xd).double(), B, groups)

        def call(T):
            _lib_call("kd_groupnorm_stats_jvp_f32", _p(T["x"]), chan, _p(T["xd"]), chan, _p(T["st"]), _p(T["js"]), B, hw[0] * hw[1], chan, groups,
                      C.c_float(1e-5))
            return T["js"], T["st"]
        return dict(ins={"x": tokens(x), "xd": tokens(xd)}, outs={"st": ((B, groups, 4), F32), "js": ((B, groups, 4), F32)}, call=call,
                    ref=lambda R: (js64, None), tol=[("abs", 2.0 ** -23 * js64.abs().max().item()), None])
    return Case("groupnorm_stats_jvp[64,7x7]", "groupnorm_stats_jvp", "unet_f32.hip", make, kernel="groupnorm_stats_jvp_f32")


def _adagn_jvp_case():
    def make(env):
        chan, hw = 64, (7, 7)
        x, xd, w, b, y64, yd64, base_y, base_yd = adagn_jvp_reference(chan, hw, False, True)
        B, groups, n = x.shape[0], chan // 32, hw[0] * hw[1]

        def call(T):
            _lib_call("kd_groupnorm_stats_jvp_f32", _p(T["x"]), chan, _p(T["xd"]), chan, _p(T["st"]), _p(T["js"]), B, n, chan, groups, C.c_float(1e-5))
            _lib_call("kd_adagn_apply_jvp_f32", _p(T["x"]), chan, _p(T["xd"]), chan, _p(T["st"]), _p(T["js"]), _p(T["wb"]), 2 * chan, _p(T["y"]), chan,
                      _p(T["yd"]), chan, B, n, chan, groups, 1)
            return T["y"], T["yd"]
        return dict(ins={"x": tokens(x), "xd": tokens(xd), "wb": torch.cat([w, b], 1)},
                    outs={"st": ((B, groups, 4), F32), "js": ((B, groups, 4), F32), "y": ((B * n, chan), F32), "yd": ((B * n, chan), F32)}, call=call,
                    ref=lambda R: (tokens(y64), tokens(yd64)), tol=[("abs", 4 * base_y), ("abs", 4 * base_yd)])
    return Case("adagn_jvp[64,7x7]", "adagn_apply_jvp", "unet_f32.hip", make, kernel="adagn_apply_jvp_f32")


def _stacked_conv_case():
    def make(env):
        ks, ci, co, hw = 3, 128, 128, (5, 9)
        B, (H, W) = 2, hw
        x, w, b, r, ref, bound = conv_reference(ks, ci, co, hw, True, True)
        # the stacked batch: the same two samples again behind the first two, without the bias
        ref_s = torch.cat([tokens(ref), tokens(ref - b.double()[None, :, None, None])])
        bound_s = torch.cat([tokens(bound), tokens(bound)])

        def call(T):
            _lib_call("kd_pack_conv_x3", _p(T["w"]), _p(T["wp"]), co, ci, ks)
            _lib_call("kd_conv2d_x3_stacked", _p(T["x"]), ci, _p(T["wp"]), _p(T["b"]), _p(T["r"]), co, _p(T["y"]), co, 2 * B, H, W, ci, co, ks, B)
            return T["y"]

        def tol(got, want):
            err = ((got.cpu().double() - want).abs() / bound_s).max().item()
            assert err < SPLIT3, f"{err:.3e} of sum|a||w|"
            return err
        return dict(ins={"x": tokens(x).repeat(2, 1), "w": w, "b": b, "r": tokens(r).repeat(2, 1)},
                    outs={"wp": ((4 * ks * ks * ci * co,), torch.uint8), "y": ((2 * B * H * W, co), F32)}, call=call, ref=lambda R: ref_s, tol=tol)
    return Case("conv2d_x3_stacked[k3,128->128,5x9]", "conv2d", "conv_x3.hip", make, mode="split3", kernel="conv2d_x3")


GUARD_CASES = [_stats_jvp_case(), _adagn_jvp_case(), _stacked_conv_case()]


@pytest.mark.parametrize("c", GUARD_CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")


# ---- 4. the model -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def jvp_reference(name):
    """(x, sigma, aug, v, (F, F_dot), (D, D_dot)) in fp64 from ``torch.func.jvp`` of the restatement: computed once."""
    cfg, _, sd = built(name)
    x, sigma, aug = ur.inputs(name)
    v = torch.randint(0, 2, x.shape, generator=torch.Generator().manual_seed(23)).float() * 2 - 1
    f = torch.func.jvp(forward_fn(sd, sigma, aug), (x.double(),), (v.double(),))
    d = torch.func.jvp(denoiser_fn(sd, sigma, cfg["model"]["sigma_data"], aug), (x.double(),), (v.double(),))
    return x, sigma, aug, v, f, d


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_jvp_matches_fp64(KD, name, monkeypatch):
    cfg, model, _ = built(name)
    x, sigma, aug, v, (f64, fd64), (d64, dd64) = jvp_reference(name)
    den = KD.Denoiser(model, cfg["model"]["sigma_data"])
    xs, ss, vs, kw = g(x), g(sigma), g(v), _kw(aug)
    with torch.no_grad():
        f, fd = model.forward_jvp(xs, ss, vs, **kw)
        d, dd = den.forward_jvp(xs, ss, vs, **kw)
        assert torch.equal(f, model(xs, ss, **kw)), "the dual pass's primal is not the forward's output"
        assert torch.equal(d, den(xs, ss, **kw)), "the dual pass's primal is not the denoiser's output"
        e_f, e_fd, e_d, e_dd = rel(f, f64), rel(fd, fd64), rel(d, d64), rel(dd, dd64)
        print(f"{name}: F {e_f:.3e}, F_dot {e_fd:.3e} (|F_dot| <= {fd64.abs().max().item():.3g}), D {e_d:.3e}, D_dot {e_dd:.3e} from the fp64 JVP (5e-4)")
        assert f.shape == fd.shape == d.shape == dd.shape == x.shape
        assert e_fd < 5e-4 and e_dd < 5e-4 and e_f < 5e-4 and e_d < 5e-4
        f2, fd2 = model.forward_jvp(xs, ss, vs, **kw)
        d2, dd2 = den.forward_jvp(xs, ss, vs, **kw)
        assert torch.equal(f, f2) and torch.equal(fd, fd2) and torch.equal(d, d2) and torch.equal(dd, dd2), "a second dual pass gives other bits"
        monkeypatch.setenv("KDIFF_GEMM", "bf16")                       # fp32-grade whatever KDIFF_GEMM says
        fb, fdb = model.forward_jvp(xs, ss, vs, **kw)
        assert torch.equal(f, fb) and torch.equal(fd, fdb)


def test_forward_jvp_keeps_the_forward_plans_and_follows_the_weights(KD):
    cfg, _, sd = built("unet_a")
    x, sigma, aug, v, _, _ = jvp_reference("unet_a")

    def fresh(state):
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(state)
        return model.to(DEV)

    def dual(model):
        with torch.no_grad():
            return model.forward_jvp(g(x), g(sigma), g(v), **_kw(aug))
    model = fresh(sd)
    inner = getattr(model, "inner_model", model)
    with torch.no_grad():
        model(g(x), g(sigma), **_kw(aug))
        model(g(x)[:1], g(sigma)[:1], **({} if aug is None else {"aug_cond": g(aug)[:1]}))
    before = dict(inner._plans)
    assert len(before) == 2
    f, fd = dual(model)
    assert list(inner._plans) == list(before) and all(inner._plans[k] is before[k] for k in before), "forward_jvp touched the forward plans"
    assert len(inner._dual_cache.plans) == 1
    plan = next(iter(inner._dual_cache.plans.values()))
    assert torch.equal(dual(model)[1], fd) and next(iter(inner._dual_cache.plans.values())) is plan          # planned once
    with torch.no_grad():
        inner.u_net.d_blocks[0][1].main[2].weight.mul_(1.5)
    f2, fd2 = dual(model)
    assert not torch.equal(fd2, fd), "the tangent did not move with the weights"
    assert next(iter(inner._dual_cache.plans.values())) is not plan and len(inner._dual_cache.plans) == 1
    want = dual(fresh(model.state_dict()))
    assert torch.equal(f2, want[0]) and torch.equal(fd2, want[1]), "not what a fresh model with these weights computes"


def test_log_likelihood_vs_fp64_cpu_solver(KD):
    """``log_likelihood(K.Denoiser(unet, sd), x, ...)`` against the same dopri5 rules in fp64 on the CPU over the restated denoiser under autograd
    (the reference's formulation); two seeded runs are identical."""
    cfg, model, sd = built("unet_b")
    mc = cfg["model"]
    torch.manual_seed(0)
    x = torch.randn(2, 1, 28, 28) * 0.5
    den = KD.Denoiser(model, mc["sigma_data"])
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        runs.append(KD.likelihood.log_likelihood(den, x.to(DEV), mc["sigma_min"], mc["sigma_max"]))
    (ll, info), (ll_again, info_again) = runs
    assert torch.equal(ll, ll_again) and info == info_again, "two seeded runs differ"
    torch.manual_seed(11)
    v = (torch.randint_like(x.to(DEV), 2) * 2 - 1).cpu().double()
    fevals = 0

    def f(t, y):
        nonlocal fevals
        fevals += 1
        sig = torch.full((2,), t, dtype=torch.float64)
        with torch.enable_grad():
            xx = y[0].detach().requires_grad_()
            d = (xx - denoiser_fn(sd, sig, mc["sigma_data"])(xx)) / t
            grad = torch.autograd.grad((d * v).sum(), xx)[0]
        return d.detach(), (v * grad).flatten(1).sum(1)
    lat, dll = KD.likelihood.dopri5(f, (x.double(), torch.zeros(2, dtype=torch.float64)), mc["sigma_min"], mc["sigma_max"], 1e-4, 1e-4, vec=_CpuVec)
    ref = torch.distributions.Normal(0.0, float(mc["sigma_max"])).log_prob(lat).flatten(1).sum(1) + dll
    print(f"unet_b: HIP ll {ll.tolist()} fevals {info['fevals']}; fp64 CPU ll {ref.tolist()} fevals {fevals}")
    assert relerr(ll, ref) < 1e-3, (ll.tolist(), ref.tolist())
    assert abs(info["fevals"] - fevals) <= 6


def test_forward_jvp_refusals_on_the_device(KD):
    cfg, model, sd = built("unet_b")
    x, sigma, _ = ur.inputs("unet_b")
    xs, ss = g(x), g(sigma)
    with torch.no_grad():
        with pytest.raises(TypeError, match="tangent"):
            model.forward_jvp(xs, ss, torch.ones_like(xs, dtype=torch.float64))
        with pytest.raises(ValueError, match="tangent"):
            model.forward_jvp(xs, ss, torch.ones_like(xs)[:, :, :14])
        with pytest.raises(RuntimeError, match="tangent"):
            model.forward_jvp(xs, ss, torch.ones_like(x))
        with pytest.raises(ValueError, match="unet_cond"):
            model.forward_jvp(xs, ss, torch.ones_like(xs), unet_cond=xs)
        with pytest.raises(ValueError, match="unet_cond"):
            KD.Denoiser(model, 0.5).forward_jvp(xs, ss, torch.ones_like(xs), unet_cond=xs)
        dropping = KD.config.make_model(KD.config.load_config({"model": dict(ur.UNET_B["model"], dropout_rate=0.1), "dataset": ur.UNET_B["dataset"]}))
        dropping = dropping.requires_grad_(False).to(DEV).train()
        with pytest.raises(NotImplementedError, match="dropout"):
            dropping.forward_jvp(xs, ss, torch.ones_like(xs))
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model.forward_jvp(xs.clone().requires_grad_(True), ss, torch.ones_like(xs))

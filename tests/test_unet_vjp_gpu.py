"""The reverse (VJP) pass of the image_v1 U-Net on the MI355X: the AdaGN and resampling reverse kernels (csrc/unet_vjp_f32.hip), the convolution's
data gradient on the existing kernel, ``forward_vjp`` of the model and of ``Denoiser`` around it, and one gradient-guidance evaluation.  Truth is
``torch.autograd.grad`` in fp64 on the CPU: of ``adagn_expr``, of ``unet_ref.downsample`` / ``upsample``, of ``F.conv2d`` and of the restatement
(tests/test_unet_jvp_cpu.py: ``forward_fn`` / ``denoiser_fn``).

Bounds.
* AdaGN reverse and the resamplers' transposes: the rule of tests/test_unet_gpu.py -- ``base`` = the error of the SAME autograd call in fp32 on the
  CPU against fp64; the kernel is allowed 4 x base.
* gstats (from the formats, as jstats): every term and both sums in fp64 over <= 8192 elements, x centred with the fp64 mean; what is left is the
  rounding of the fp32 rstd the kernel is handed (2^-24, and the means are at most linear in it) and one fp32 rounding of the result (2^-24):
  2^-23 of the largest.
* conv data gradient: the forward conv's own bound, |got - ref| / sum |g| |w| < 2^-14 per output.
* model: the output is the forward's bits; the pullback is within 5e-4 (max-abs relative, the forward's and the dual pass's gate) of fp64 autograd,
  for F and for D; linear in grad_out to 1e-5.
* adjoint identity against the dual pass: |<J v, u> - <v, J^T u>| <= 5e-4 (max|J v| sum|u| + max|J^T u| sum|v|), which is what the two 5e-4 gates
  allow the two sides together.
"""
import ctypes as C
import functools

import pytest
import torch
from torch.nn import functional as F

from tests import unet_ref as ur
from tests.guard import Case, run_case
from tests.test_unet_gpu import (DEV, F32, K_DOWN, K_UP, SPLIT3, _kw, _lib_call, _p, adagn_expr, adagn_reference, built, conv_reference, g, nchw,
                                 rel, rn, tokens, within)
from tests.test_unet_jvp_cpu import denoiser_fn, forward_fn

pytestmark = pytest.mark.gpu


def pm1(shape, seed):
    return torch.randint(0, 2, tuple(shape), generator=torch.Generator().manual_seed(seed)).float() * 2 - 1


# ---- 1. AdaGN reverse ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def adagn_vjp_reference(chan, hw, shifted, gelu):
    """(x, w, b, g_y, g_add, g_x in fp64 without g_add, base, gstats in fp64): the fp64 gradient of ``adagn_expr`` w.r.t. x and the fp32 call's
    own error, computed once."""
    B, (H, W), groups = 3, hw, chan // 32
    x, w, b, _, _ = adagn_reference(chan, hw, shifted, gelu)
    seed = chan + 3 * H + (50 if shifted else 0)
    gy, ga = rn(B, chan, H, W, seed=seed + 17), rn(B, chan, H, W, seed=seed + 18)

    def grad(x, w, b, gy):
        x = x.clone().requires_grad_(True)
        return torch.autograd.grad(adagn_expr(x, w, b, groups, gelu), x, gy)[0]
    gx64 = grad(x.double(), w.double(), b.double(), gy.double())
    base = (grad(x, w, b, gy).double() - gx64).abs().max().item()
    # the two group means, from the normalised activation on
    xh = F.group_norm(x.double(), groups, eps=1e-5).requires_grad_(True)
    pre = torch.addcmul(b.double()[:, :, None, None], xh, w.double()[:, :, None, None] + 1)
    gxh = torch.autograd.grad(F.gelu(pre) if gelu else pre, xh, gy.double())[0]
    per_group = lambda t: t.reshape(B, groups, -1).mean(-1)
    m1, m2 = per_group(gxh), per_group(gxh * xh.detach())
    return x, w, b, gy, ga, gx64, base, torch.stack([m1, m2, torch.zeros_like(m1), torch.zeros_like(m1)], dim=-1)


@pytest.mark.parametrize("with_add", [False, True], ids=["", "g_add"])
@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "plain"])
@pytest.mark.parametrize("chan,hw,shifted,layout", [(64, (7, 7), False, "plain"), (128, (16, 16), False, "wide"), (64, (16, 16), True, "inplace"),
                                                    (128, (7, 7), True, "plain"), (64, (2, 2), False, "plain")], ids=str)
def test_adagn_vjp_matches_fp64(KD, chan, hw, shifted, layout, gelu, with_add):
    uo = KD.unet_ops
    B, (H, W), groups = 3, hw, chan // 32
    x, w, b, gy, ga, gx64, base, gs64 = adagn_vjp_reference(chan, hw, shifted, gelu)
    want = gx64 + ga.double() if with_add else gx64
    rows = B * H * W
    xt, gyt, gat, wb = g(tokens(x)), g(tokens(gy)), g(tokens(ga)) if with_add else None, g(torch.cat([w, b], dim=1))
    stats = uo.groupnorm_stats(xt, B, groups)
    fill = None

    def operands():
        if layout == "wide":    # inputs: the right halves of NaN-filled [rows, 2 C] buffers; the output: the left half of a buffer whose right half stays
            ins = []
            for t in (xt, gyt, gat):
                buf = None if t is None else torch.full((rows, 2 * chan), float("nan"), device=DEV)
                if buf is not None:
                    buf[:, chan:] = t
                ins.append(None if buf is None else buf[:, chan:])
            out = torch.full((rows, 2 * chan), -7.0, device=DEV)
            return (*ins, out[:, :chan], out)
        if layout == "inplace":                                         # g_x over g_y
            gin = gyt.clone()
            return xt, gin, gat, gin, None
        return xt, gyt, gat, None, None
    xin, gin, ain, out, fill = operands()
    gstats = uo.adagn_vjp_stats(xin, stats, wb, gin, gelu=gelu)
    assert torch.equal(gstats, uo.adagn_vjp_stats(xin, stats, wb, gin, gelu=gelu)), "a repeat of the statistics gives other bits"
    gx = uo.adagn_vjp_apply(xin, stats, gstats, wb, gin, g_add=ain, gelu=gelu, out=out)
    what = f"adagn vjp C{chan} {H}x{W} shifted={shifted} gelu={gelu} g_add={with_add} {layout}"
    e_gs = (gstats.cpu().double() - gs64).abs().max().item() / gs64.abs().max().item()
    print(f"{what}: gstats {e_gs:.3e} of the largest ({2.0 ** -23:.3e})")
    assert e_gs < 2.0 ** -23
    assert bool((gstats[..., 2:] == 0).all())
    within(nchw(gx, B, H, W), want, base, what)
    if fill is not None:
        assert bool((fill[:, chan:] == -7.0).all()), "the columns beside the output range were written"
    if layout == "inplace":
        assert gx.data_ptr() == gin.data_ptr()
    xin, gin, ain, out, _ = operands()
    assert torch.equal(uo.adagn_vjp_apply(xin, stats, gstats, wb, gin, g_add=ain, gelu=gelu, out=out), gx), "a repeat gives other bits"
    if with_add and layout == "plain":                                  # g_x over g_add
        acc = gat.clone()
        assert torch.equal(uo.adagn_vjp_apply(xt, stats, gstats, wb, gyt, g_add=acc, gelu=gelu, out=acc), gx)


def test_adagn_vjp_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    x, gy, wb = g(rn(2 * 4, 64)), g(rn(2 * 4, 64, seed=1)), g(rn(2, 128))
    stats = uo.groupnorm_stats(x, 2, 2)
    with pytest.raises(ValueError, match="g_y shape"):
        uo.adagn_vjp_stats(x, stats, wb, gy[:4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.adagn_vjp_stats(x, stats, wb, gy.cpu())
    with pytest.raises(RuntimeError, match="multiple of 4"):
        uo.adagn_vjp_stats(x, uo.groupnorm_stats(x, 2, 32), wb, gy)
    gstats = uo.adagn_vjp_stats(x, stats, wb, gy)
    with pytest.raises(RuntimeError, match="not x"):
        uo.adagn_vjp_apply(x, stats, gstats, wb, gy, out=x)
    with pytest.raises(ValueError, match="gstats"):
        uo.adagn_vjp_apply(x, stats, gstats[:1], wb, gy)


# ---- 2. the resamplers' transposes ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def resample_vjp_reference(up, hw):
    """(g_y, acc, g_x in fp64, g_x + acc in fp64, base, base with acc): fp64 autograd of the restatement's resampler at input size hw."""
    B, chan, (H, W) = 2, 64, hw
    fn, kern = (ur.upsample, K_UP) if up else (ur.downsample, K_DOWN)
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2)
    gy, acc = rn(B, chan, Ho, Wo, seed=H * 31 + W + (5 if up else 0)), rn(B, chan, H, W, seed=H * 37 + W)

    def grad(gy, dtype):
        x = torch.zeros(B, chan, H, W, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(fn(x, kern), x, gy.to(dtype))[0]
    g64, g32 = grad(gy, torch.float64), grad(gy, torch.float32)
    return gy, acc, g64, g64 + acc.double(), (g32.double() - g64).abs().max().item(), ((g32 + acc).double() - (g64 + acc.double())).abs().max().item()


@pytest.mark.parametrize("up", [False, True], ids=["down2", "up2"])
@pytest.mark.parametrize("hw", [(2, 2), (4, 6), (6, 10)], ids=str)             # (2, 2): every tap reflects
def test_resample_vjp_matches_fp64(KD, hw, up):
    uo = KD.unet_ops
    B, chan, (H, W) = 2, 64, hw
    gy, acc, g64, g64_acc, base, base_acc = resample_vjp_reference(up, hw)
    fn, name = (uo.up2_vjp, "up2_vjp") if up else (uo.down2_vjp, "down2_vjp")
    gyt = g(tokens(gy))
    gx = fn(gyt, B, H, W)
    within(nchw(gx, B, H, W), g64, base, f"{name} {H}x{W}")
    assert torch.equal(gx, fn(gyt, B, H, W)), "a repeat gives other bits"
    # into the right half of a wider buffer, added to what it holds; the input a column range too
    buf = torch.full((B * H * W, 2 * chan), -3.0, device=DEV)
    buf[:, chan:] = g(tokens(acc))
    src = torch.full((gyt.shape[0], 2 * chan), float("nan"), device=DEV)
    src[:, :chan] = gyt
    out = fn(src[:, :chan], B, H, W, out=buf[:, chan:], accumulate=True)
    within(nchw(out, B, H, W), g64_acc, base_acc, f"{name} {H}x{W} accumulate")
    assert bool((buf[:, :chan] == -3.0).all()), "the columns beside the output range were written"
    # without the flag the sum replaces what the range held
    assert torch.equal(fn(gyt, B, H, W, out=buf[:, chan:]), gx)
    # the transpose for real: <down2(x), g_y> == <x, down2_vjp(g_y)> on the kernels themselves, to fp32 rounding of sums of H W C terms
    x = g(rn(B * H * W, chan, seed=3))
    y = (uo.up2 if up else uo.down2)(x, B, H, W)
    lhs, rhs = (y.double() * gyt.double()).sum().item(), (x.double() * gx.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * (y.double() * gyt.double()).abs().sum().item(), (lhs, rhs)


def test_resample_vjp_refuses_odd_and_tiny(KD):
    uo = KD.unet_ops
    with pytest.raises(RuntimeError, match="must be even"):
        uo.down2_vjp(g(rn(2 * 1 * 2, 64)), 2, 3, 4)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        uo.up2_vjp(g(rn(2 * 2 * 8, 64)), 2, 1, 4)
    with pytest.raises(ValueError, match="accumulate"):
        uo.up2_vjp(g(rn(2 * 4 * 4, 64)), 2, 2, 2, accumulate=True)
    with pytest.raises(ValueError, match="rows"):
        uo.down2_vjp(g(rn(2 * 2 * 2, 64)), 2, 4, 4, out=g(rn(2 * 4 * 4 - 1, 64)))


# ---- 3. the convolution's data gradient ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def conv_dgrad_reference(ks, ci, co, hw):
    """(w, g_y, g_x in fp64, sum |g| |w| per output): fp64 autograd of ``F.conv2d`` on the forward test's weights."""
    B, (H, W) = 2, hw
    _, w, *_ = conv_reference(ks, ci, co, hw, False, False)
    gy = rn(B, co, H, W, seed=100 * ks + ci + co + 7 * H + W + 21) * torch.logspace(-3, 3, co)[None, :, None, None]

    def grad(w, gy):
        x = torch.zeros(B, ci, H, W, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(F.conv2d(x, w.double(), padding=ks // 2), x, gy.double())[0]
    return w, gy, grad(w, gy), grad(w.abs(), gy.abs())


@pytest.mark.parametrize("ks,ci,co,hw", [(3, 64, 128, (7, 7)), (1, 128, 384, (5, 9)), (3, 128, 128, (5, 9))], ids=lambda v: str(v).replace(" ", ""))
def test_conv_dgrad_error_is_bounded(KD, ks, ci, co, hw):
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    w, gy, ref, bound = conv_dgrad_reference(ks, ci, co, hw)
    wt, gyt = g(w), g(tokens(gy))
    gx = uo.conv2d_dgrad(gyt, wt, B, H, W)
    err = ((nchw(gx.cpu().double(), B, H, W) - ref).abs() / bound).max().item()
    print(f"conv dgrad k{ks} {ci}->{co} {H}x{W}: {err:.3e} of sum|g||w| (bound {SPLIT3:.3e})")
    assert err < SPLIT3
    # it is the forward kernel on the transposed, flipped weight
    assert torch.equal(gx, uo.conv2d(gyt, wt.flip(2, 3).transpose(0, 1).contiguous(), B, H, W))
    # + residual, into a column range, from a column range
    rbuf = torch.full((B * H * W, 2 * ci), -7.0, device=DEV)
    r = g(rn(B * H * W, ci, seed=5))
    rbuf[:, ci:] = r
    src = torch.full((B * H * W, co + 64), float("nan"), device=DEV)
    src[:, 64:] = gyt
    acc = uo.conv2d_dgrad(src[:, 64:], wt, B, H, W, residual=rbuf[:, ci:], out=rbuf[:, ci:])
    err = ((nchw(acc.cpu().double(), B, H, W) - ref - nchw(r.cpu().double(), B, H, W)).abs() / (bound + nchw(r.cpu().double(), B, H, W).abs())).max().item()
    assert err < SPLIT3 and bool((rbuf[:, :ci] == -7.0).all())
    # the packed image: one per weight tensor and version
    img = uo.pack_conv_dgrad(wt)
    assert uo.pack_conv_dgrad(wt) is img and uo.pack_conv_dgrad(wt, q_rows=64) is not img
    # q_rows: the first rows of the weight carry 1 / 8, as the forward folds it into a qkv projection
    folded = wt.clone()
    folded[:64] *= 0.125
    assert torch.equal(uo.conv2d_dgrad(gyt, wt, B, H, W, q_rows=64), uo.conv2d_dgrad(gyt, folded, B, H, W))
    wt.mul_(1.5)
    assert uo.pack_conv_dgrad(wt) is not img
    assert not torch.equal(uo.conv2d_dgrad(gyt, wt, B, H, W), gx)


# ---- 4. guard bands: one ragged shape per new entry point ----------------------------------------------------------------------------------------

def _adagn_vjp_case(apply):
    def make(env):
        chan, hw = 64, (7, 7)
        x, w, b, gy, ga, gx64, base, gs64 = adagn_vjp_reference(chan, hw, False, True)
        B, groups, n = x.shape[0], chan // 32, hw[0] * hw[1]

        def call(T):
            _lib_call("kd_groupnorm_stats_f32", _p(T["x"]), chan, _p(T["st"]), B, n, chan, groups, C.c_float(1e-5))
            _lib_call("kd_adagn_vjp_stats_f32", _p(T["x"]), chan, _p(T["st"]), _p(T["wb"]), 2 * chan, _p(T["gy"]), chan, _p(T["gs"]), B, n, chan, groups, 1)
            if not apply:
                return T["gs"], T["st"]
            _lib_call("kd_adagn_vjp_apply_f32", _p(T["x"]), chan, _p(T["st"]), _p(T["gs"]), _p(T["wb"]), 2 * chan, _p(T["gy"]), chan, _p(T["ga"]), chan,
                      _p(T["gx"]), chan, B, n, chan, groups, 1)
            return T["gx"], T["gs"]
        ins = {"x": tokens(x), "wb": torch.cat([w, b], 1), "gy": tokens(gy)}
        outs = {"st": ((B, groups, 4), F32), "gs": ((B, groups, 4), F32)}
        gs_tol = ("abs", 2.0 ** -23 * gs64.abs().max().item())
        if not apply:
            return dict(ins=ins, outs=outs, call=call, ref=lambda R: (gs64, None), tol=[gs_tol, None])
        return dict(ins=dict(ins, ga=tokens(ga)), outs=dict(outs, gx=((B * n, chan), F32)), call=call,
                    ref=lambda R: (tokens(gx64 + ga.double()), gs64), tol=[("abs", 4 * base), gs_tol])
    name = "adagn_vjp_apply" if apply else "adagn_vjp_stats"
    return Case(f"{name}[64,7x7]", name, "unet_vjp_f32.hip", make, kernel=name + "_f32")


def _resample_vjp_case(up):
    def make(env):
        B, chan, H, W = 2, 64, 4, 6
        gy, _, g64, _, base, _ = resample_vjp_reference(up, (H, W))

        def call(T):
            _lib_call("kd_up2_vjp_f32" if up else "kd_down2_vjp_f32", _p(T["gy"]), chan, _p(T["gx"]), chan, B, H, W, chan, 0)
            return T["gx"]
        return dict(ins={"gy": tokens(gy)}, outs={"gx": ((B * H * W, chan), F32)}, call=call, ref=lambda R: tokens(g64), tol=("abs", 4 * base))
    name = "up2_vjp" if up else "down2_vjp"
    return Case(f"{name}[4x6]", name, "unet_vjp_f32.hip", make, kernel=name + "_f32")


GUARD_CASES = [_adagn_vjp_case(False), _adagn_vjp_case(True), _resample_vjp_case(False), _resample_vjp_case(True)]


@pytest.mark.parametrize("c", GUARD_CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")


# ---- 5. the model --------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def vjp_reference(name):
    """(x, sigma, aug, u, J_F^T u, J_D^T u) in fp64 from ``torch.autograd.grad`` of the restatement: computed once."""
    cfg, _, sd = built(name)
    x, sigma, aug = ur.inputs(name)
    u = pm1(x.shape, 29)

    def grad(fn):
        xx = x.double().requires_grad_(True)
        return torch.autograd.grad(fn(xx), xx, u.double())[0]
    return x, sigma, aug, u, grad(forward_fn(sd, sigma, aug)), grad(denoiser_fn(sd, sigma, cfg["model"]["sigma_data"], aug))


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_vjp_matches_fp64(KD, name, monkeypatch):
    cfg, model, _ = built(name)
    x, sigma, aug, u, gf64, gd64 = vjp_reference(name)
    den = KD.Denoiser(model, cfg["model"]["sigma_data"])
    xs, ss, us, kw = g(x), g(sigma), g(u), _kw(aug)
    f, pb_f = model.forward_vjp(xs, ss, **kw)                           # grad mode on: nothing here requires grad, and no graph is built
    d, pb_d = den.forward_vjp(xs, ss, **kw)
    gf, gd = pb_f(us), pb_d(us)
    assert not f.requires_grad and not gf.requires_grad and f.grad_fn is None and gf.grad_fn is None
    with torch.no_grad():
        assert torch.equal(f, model(xs, ss, **kw)), "forward_vjp's output is not the forward's"
        assert torch.equal(d, den(xs, ss, **kw)), "forward_vjp's output is not the denoiser's"
        e_f, e_d = rel(gf, gf64), rel(gd, gd64)
        print(f"{name}: J_F^T u {e_f:.3e} (|.| <= {gf64.abs().max().item():.3g}), J_D^T u {e_d:.3e} from fp64 autograd (5e-4)")
        assert gf.shape == gd.shape == x.shape
        assert e_f < 5e-4 and e_d < 5e-4
        assert torch.equal(pb_f(us), gf) and torch.equal(pb_d(us), gd), "a second pullback gives other bits"
        f2, pb_f2 = model.forward_vjp(xs, ss, **kw)
        d2, pb_d2 = den.forward_vjp(xs, ss, **kw)
        assert torch.equal(f2, f) and torch.equal(d2, d) and torch.equal(pb_f2(us), gf) and torch.equal(pb_d2(us), gd), "a second pass gives other bits"
        assert torch.equal(pb_f(us), gf), "an earlier pullback changed when a later primal ran"
        # linear in grad_out
        e_lin = max(rel(pb_f(2 * us), 2 * gf.cpu()), rel(pb_d(2 * us), 2 * gd.cpu()))
        print(f"{name}: linearity {e_lin:.3e} (1e-5)")
        assert e_lin < 1e-5
        w = g(pm1(x.shape, 31))
        assert torch.equal(pb_f(w), pb_f2(w)) and not torch.equal(pb_f(w), gf), "another grad_out through the same pullback"
        monkeypatch.setenv("KDIFF_GEMM", "bf16")                       # fp32-grade whatever KDIFF_GEMM says
        fb, pb_b = model.forward_vjp(xs, ss, **kw)
        assert torch.equal(fb, f) and torch.equal(pb_b(us), gf)


# ---- 6. the adjoint identity against the dual pass -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_pullback_is_the_adjoint_of_the_dual_pass(KD, name):
    cfg, model, _ = built(name)
    x, sigma, aug = ur.inputs(name)
    den = KD.Denoiser(model, cfg["model"]["sigma_data"])
    u, v = pm1(x.shape, 29), pm1(x.shape, 23)
    xs, ss, us, vs, kw = g(x), g(sigma), g(u), g(v), _kw(aug)
    with torch.no_grad():
        for what, net in (("F", model), ("D", den)):
            jv = net.forward_jvp(xs, ss, vs, **kw)[1].double()
            jtu = net.forward_vjp(xs, ss, **kw)[1](us).double()
            lhs, rhs = (jv * us.double()).sum().item(), (vs.double() * jtu).sum().item()
            bound = 5e-4 * (jv.abs().max().item() * u.abs().sum().item() + jtu.abs().max().item() * v.abs().sum().item())
            print(f"{name} {what}: <J v, u> = {lhs:.9g}, <v, J^T u> = {rhs:.9g}, difference {abs(lhs - rhs):.3e} (bound {bound:.3e})")
            assert abs(lhs - rhs) <= bound


# ---- 7. plans and weights ------------------------------------------------------------------------------------------------------------------------

def test_forward_vjp_keeps_the_plans_and_follows_the_weights(KD):
    cfg, _, sd = built("unet_a")
    x, sigma, aug, u, _, _ = vjp_reference("unet_a")

    def fresh(state):
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(state)
        return model.to(DEV)
    model = fresh(sd)
    inner = getattr(model, "inner_model", model)
    with torch.no_grad():
        model(g(x), g(sigma), **_kw(aug))
        model(g(x)[:1], g(sigma)[:1], **({} if aug is None else {"aug_cond": g(aug)[:1]}))
        model.forward_jvp(g(x), g(sigma), g(u), **_kw(aug))
    plans, duals = dict(inner._plans), dict(inner._dual_cache.plans)
    assert len(plans) == 2 and len(duals) == 1
    out, pullback = model.forward_vjp(g(x), g(sigma), **_kw(aug))
    grad = pullback(g(u))
    for cache, before in ((inner._plans, plans), (inner._dual_cache.plans, duals)):
        assert list(cache) == list(before) and all(cache[k] is before[k] for k in before), "forward_vjp touched the forward's or the dual pass's plans"
    consts = dict(inner._vjp_cache.plans)
    assert len(consts) == 1
    model.forward_vjp(g(x), g(sigma), **_kw(aug))
    assert dict(inner._vjp_cache.plans) == consts                       # derived once
    with torch.no_grad():
        inner.u_net.d_blocks[0][1].main[2].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="weights changed"):
        pullback(g(u))
    out2, pullback2 = model.forward_vjp(g(x), g(sigma), **_kw(aug))
    grad2 = pullback2(g(u))
    assert not torch.equal(grad2, grad), "the gradient did not move with the weights"
    assert len(inner._vjp_cache.plans) == 1 and next(iter(inner._vjp_cache.plans.values())) is not next(iter(consts.values()))
    for cache, before in ((inner._plans, plans), (inner._dual_cache.plans, duals)):
        assert list(cache) == list(before) and all(cache[k] is before[k] for k in before)
    want, want_pullback = fresh(model.state_dict()).forward_vjp(g(x), g(sigma), **_kw(aug))
    assert torch.equal(out2, want) and torch.equal(grad2, want_pullback(g(u))), "not what a fresh model with these weights computes"


# ---- 8. use: one gradient-guidance evaluation ----------------------------------------------------------------------------------------------------

def test_reconstruction_guidance_gradient(KD):
    """d/dx sum(mask (D(x, sigma) - target)^2): the denoised image and the pullback from one ``forward_vjp``."""
    cfg, model, sd = built("unet_b")
    sdata = cfg["model"]["sigma_data"]
    x, sigma, aug = ur.inputs("unet_b")
    target = rn(*x.shape, seed=41)
    mask = (rn(*x.shape, seed=42) > 0).float()
    xx = x.double().requires_grad_(True)
    loss = (mask.double() * (denoiser_fn(sd, sigma, sdata, aug)(xx) - target.double()) ** 2).sum()
    ref = torch.autograd.grad(loss, xx)[0]
    den = KD.Denoiser(model, sdata)
    denoised, pb = den.forward_vjp(g(x), g(sigma), **_kw(aug))
    grad = pb(2 * (denoised - g(target)) * g(mask))
    err = rel(grad, ref)
    print(f"unet_b: guidance gradient {err:.3e} from fp64 autograd (5e-4), |grad| <= {ref.abs().max().item():.3g}")
    assert grad.shape == x.shape and err < 5e-4


# ---- 9. refusals on the device -------------------------------------------------------------------------------------------------------------------

def test_forward_vjp_refusals_on_the_device(KD):
    cfg, model, sd = built("unet_b")
    x, sigma, _ = ur.inputs("unet_b")
    xs, ss = g(x), g(sigma)
    with torch.no_grad():
        for net in (model, KD.Denoiser(model, 0.5)):
            _, pb = net.forward_vjp(xs, ss)
            with pytest.raises(ValueError, match="grad_out"):
                pb(torch.ones_like(xs)[:, :, :14])
            with pytest.raises(ValueError, match="grad_out"):
                pb(None)
            with pytest.raises(TypeError, match="grad_out"):
                pb(torch.ones_like(xs, dtype=torch.float64))
            with pytest.raises(RuntimeError, match="grad_out"):
                pb(torch.ones_like(x))
            with pytest.raises(ValueError, match="unet_cond"):
                net.forward_vjp(xs, ss, unet_cond=xs)
        with pytest.raises(ValueError, match="input size 28x30"):
            model.forward_vjp(g(torch.zeros(2, 1, 28, 30)), ss)
        dropping = KD.config.make_model(KD.config.load_config({"model": dict(ur.UNET_B["model"], dropout_rate=0.1), "dataset": ur.UNET_B["dataset"]}))
        dropping = dropping.requires_grad_(False).to(DEV).train()
        with pytest.raises(NotImplementedError, match="dropout"):
            dropping.forward_vjp(xs, ss)
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model.forward_vjp(xs.clone().requires_grad_(True), ss)

"""The image_v1 U-Net on the MI355X (csrc/conv_x3.hip, csrc/unet_f32.hip, K.unet_ops, K.models.image_v1).  Truth is fp64 on the CPU.

Bounds.
* conv: the split-bf16x3 bound of tests/test_ops_gpu.py::test_split3_error_is_bounded_and_asymmetric_safe, |got - ref| / sum |a| |w| < 2^-14, on
  operands whose channels span six / four decades.
* AdaGN, resample, proj_in / proj_out, cond MLP: the rule of tests/test_augment_gpu.py -- ``base`` = the largest absolute difference between the
  SAME torch expression in fp32 and in fp64 on those inputs; the kernel is allowed 4 x base.  Both values are printed.
* group-norm statistics (from the formats): mean_hi + mean_lo carries the fp64 mean to 2^-47 relative, the fp64 sums over <= 8192 elements add
  < 1e-12, so 1e-10 relative; rstd is one fp32 rounding (2^-24) of a value whose variance (E x^2 - mean^2 in fp64, |mean| <= 100 sigma) is
  good to 1e-10, so 2^-23 relative.
* model: 5e-4 against the fp64 restatement (PLAN_BOUND["split3"] of tests/test_launch_config_gpu.py), 1e-3 against the reference's recorded fp32 output and for a
  6-step DPM++(2M) trajectory, 1e-6 between the fused and the unfused preconditioning.
"""
import ctypes as C
import functools
import json
import os

import pytest
import torch
from torch.nn import functional as F

from k_diffusion_amd import _native as nat
from tests import unet_ref as ur
from tests.guard import Case, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
SPLIT3 = 2.0 ** -14


def g(t):
    return t.to(DEV, F32).contiguous()


def rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def tokens(x):
    """NCHW -> [B H W, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def within(got, ref64, base, what):
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: error {err:.3e}, base {base:.3e}, bound {4 * base:.3e}")
    assert base > 0
    assert err <= 4 * base, f"{what}: error {err:.3e} above 4 x base = {4 * base:.3e}"


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. convolution -------------------------------------------------------------------------------------------------------------------------

SIZES = [(7, 7), (8, 8), (5, 9), (14, 14)]
# (ks, c_in, c_out): every size with every channel pair; bias / residual / wide strides rotate over the table so that each occurs with each ks
CONV_CASES = [(ks, ci, co, hw, (i + j) % 2 == 0, (i + 2 * j) % 3 == 0, (i + j) % 3 == 1)
              for j, (ks, ci, co) in enumerate([(3, 64, 128), (3, 384, 64), (3, 128, 128), (1, 128, 384)]) for i, hw in enumerate(SIZES)]
# the launcher takes N tiles of 128 where c_out allows and of 64 otherwise: the 1 x 1 kernel with the 64-wide tile too
CONV_CASES += [(1, 64, 192, (7, 7), True, False, True), (1, 64, 192, (5, 9), False, True, False)]


@functools.lru_cache(maxsize=None)
def conv_reference(ks, ci, co, hw, bias, residual):
    B, (H, W) = 2, hw
    seed = 100 * ks + ci + co + 7 * H + W
    x = rn(B, ci, H, W, seed=seed) * torch.logspace(-3, 3, ci)[None, :, None, None]
    w = rn(co, ci, ks, ks, seed=seed + 1) * torch.logspace(2, -2, co)[:, None, None, None] / (ks * ci ** 0.5)
    b = rn(co, seed=seed + 2) if bias else None
    r = rn(B, co, H, W, seed=seed + 3) if residual else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=ks // 2)
    if r is not None:
        ref = ref + r.double()
    bound = F.conv2d(x.abs().double(), w.abs().double(), padding=ks // 2)
    return x, w, b, r, ref, bound


@pytest.mark.parametrize("ks,ci,co,hw,bias,residual,wide", CONV_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv_error_is_bounded(KD, ks, ci, co, hw, bias, residual, wide):
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    x, w, b, r, ref, bound = conv_reference(ks, ci, co, hw, bias, residual)
    rows = B * H * W
    if wide:                 # the concat halves: x is the right half of a [rows, 2 ci] buffer, y the left half of a [rows, co + 64] one
        xbuf = torch.full((rows, 2 * ci), float("nan"), device=DEV)
        xbuf[:, ci:] = g(tokens(x))
        xt = xbuf[:, ci:]
        ybuf = torch.full((rows, co + 64), -7.0, device=DEV)
        out = ybuf[:, :co]
    else:
        xt, out, ybuf = g(tokens(x)), None, None
    y = uo.conv2d(xt, g(w), B, H, W, bias=None if b is None else g(b), residual=None if r is None else g(tokens(r)), out=out)
    got = nchw(y.cpu().double(), B, H, W)
    err = ((got - ref).abs() / bound).max().item()
    print(f"conv k{ks} {ci}->{co} {H}x{W} bias={bias} res={residual} wide={wide}: {err:.3e} of sum|a||w| (bound {SPLIT3:.3e})")
    assert err < SPLIT3
    if wide:
        assert bool((ybuf[:, co:] == -7.0).all()), "the columns beside the output range were written"
    assert torch.equal(y, uo.conv2d(xt, g(w), B, H, W, bias=None if b is None else g(b), residual=None if r is None else g(tokens(r))))


@pytest.mark.parametrize("ks,hw", [(3, (7, 7)), (3, (8, 8)), (1, (5, 9))])
def test_conv_never_reads_the_neighbouring_sample(KD, ks, hw):
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    x, w, *_ = conv_reference(ks, 128, 128 if ks == 3 else 384, hw, False, False)
    xt = g(tokens(x)).view(B, H * W, -1)
    base = uo.conv2d(xt.view(B * H * W, -1), g(w), B, H, W).view(B, H * W, -1)
    for other, fill in ((0, 1e30), (1, float("nan"))):
        x2 = xt.clone()
        x2[other] = fill
        y2 = uo.conv2d(x2.view(B * H * W, -1), g(w), B, H, W).view(B, H * W, -1)
        assert torch.equal(y2[1 - other], base[1 - other]), f"sample {1 - other} changed when sample {other} was filled with {fill}"


def test_conv_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    with pytest.raises(RuntimeError, match="multiples of 64"):
        uo.conv2d(g(rn(8, 32)), g(rn(64, 32, 1, 1)), 2, 2, 2)
    with pytest.raises(RuntimeError, match="kernel size"):
        uo.conv2d(g(rn(8, 64)), g(rn(64, 64, 5, 5)), 2, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.conv2d(rn(8, 64), g(rn(64, 64, 1, 1)), 2, 2, 2)
    w = g(rn(64, 64, 3, 3))
    img = uo.pack_conv(w)
    assert uo.pack_conv(w) is img                       # cached per tensor and version
    w.mul_(2.0)
    assert uo.pack_conv(w) is not img


# ---- 2. AdaGN ---------------------------------------------------------------------------------------------------------------------------------

def adagn_expr(x, w, b, groups, gelu):
    y = torch.addcmul(b[:, :, None, None], F.group_norm(x, groups, eps=1e-5), w[:, :, None, None] + 1)
    return F.gelu(y) if gelu else y


@functools.lru_cache(maxsize=None)
def adagn_reference(chan, hw, shifted, gelu):
    B, (H, W) = 3, hw
    seed = chan + 3 * H + (50 if shifted else 0)
    x = rn(B, chan, H, W, seed=seed) + (100.0 if shifted else 0.0)
    w, b = 0.3 * rn(B, chan, seed=seed + 1), 0.3 * rn(B, chan, seed=seed + 2)
    y64 = adagn_expr(x.double(), w.double(), b.double(), chan // 32, gelu)
    base = (adagn_expr(x, w, b, chan // 32, gelu).double() - y64).abs().max().item()
    return x, w, b, y64, base


@pytest.mark.parametrize("chan,hw,shifted,gelu", [(64, (7, 7), False, True), (128, (7, 7), False, False), (64, (16, 16), False, False),
                                                  (128, (16, 16), False, True), (64, (16, 16), True, True), (128, (7, 7), True, False)], ids=str)
def test_adagn_matches_fp64(KD, chan, hw, shifted, gelu):
    uo = KD.unet_ops
    B, (H, W) = 3, hw
    x, w, b, y64, base = adagn_reference(chan, hw, shifted, gelu)
    xt = g(tokens(x))
    stats = uo.groupnorm_stats(xt, B, chan // 32)
    xg = x.double().reshape(B, chan // 32, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    st = stats.cpu().double()
    e_mean = ((st[..., 0] + st[..., 1] - mean).abs() / mean.abs().clamp_min(1.0)).max().item()
    e_rstd = (st[..., 2] * (var + 1e-5).sqrt() - 1).abs().max().item()
    print(f"stats C{chan} {H}x{W} shifted={shifted}: mean {e_mean:.3e} (1e-10), rstd {e_rstd:.3e} ({2.0 ** -23:.3e})")
    assert e_mean < 1e-10 and e_rstd < 2.0 ** -23
    y = uo.adagn_apply(xt, stats, g(torch.cat([w, b], dim=1)), gelu=gelu)
    within(nchw(y, B, H, W), y64, base, f"adagn C{chan} {H}x{W} shifted={shifted} gelu={gelu}")
    assert torch.equal(stats, uo.groupnorm_stats(xt, B, chan // 32))


# ---- 3. resampling -----------------------------------------------------------------------------------------------------------------------------

K_DOWN = torch.tensor([[1 / 8, 3 / 8, 3 / 8, 1 / 8]])
K_DOWN = K_DOWN.T @ K_DOWN
K_UP = 4 * K_DOWN


@pytest.mark.parametrize("hw", [(2, 6), (6, 14), (14, 2), (2, 2), (6, 6), (14, 14)], ids=str)
def test_resample_matches_fp64(KD, hw):
    uo = KD.unet_ops
    B, chan, (H, W) = 2, 64, hw
    x = rn(B, chan, H, W, seed=H * 31 + W)
    xt = g(tokens(x))
    d64, u64 = ur.downsample(x.double(), K_DOWN), ur.upsample(x.double(), K_UP)
    d = uo.down2(xt, B, H, W)
    within(nchw(d, B, H // 2, W // 2), d64, (ur.downsample(x, K_DOWN).double() - d64).abs().max().item(), f"down2 {H}x{W}")
    # through row strides: into the left half of a wider buffer
    buf = torch.full((B * 4 * H * W, 2 * chan), -3.0, device=DEV)
    u = uo.up2(xt, B, H, W, out=buf[:, :chan])
    within(nchw(u, B, 2 * H, 2 * W), u64, (ur.upsample(x, K_UP).double() - u64).abs().max().item(), f"up2 {H}x{W}")
    assert bool((buf[:, chan:] == -3.0).all())


def test_resample_refuses_odd_and_tiny(KD):
    uo = KD.unet_ops
    with pytest.raises(RuntimeError, match="must be even"):
        uo.down2(g(rn(2 * 3 * 4, 64)), 2, 3, 4)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        uo.up2(g(rn(2 * 1 * 4, 64)), 2, 1, 4)


# ---- 4. proj_in / proj_out, cond MLP ----------------------------------------------------------------------------------------------------------

def scalings(sigma, sd):
    var = sigma ** 2 + sd ** 2
    return sd ** 2 / var, sigma * sd / var ** 0.5, 1 / var ** 0.5


@pytest.mark.parametrize("c_img,chan,hw,pre", [(3, 64, (5, 9), True), (1, 128, (7, 7), True), (3, 128, (6, 6), False), (1, 64, (2, 3), False)], ids=str)
def test_proj_in_and_out_match_fp64(KD, c_img, chan, hw, pre):
    uo = KD.unet_ops
    B, (H, W), sd = 3, hw, 0.5
    img, sigma = rn(B, c_img, H, W, seed=chan + H) * 3, torch.tensor([0.02, 1.5, 70.0])
    w_in, b_in = rn(chan, c_img, 1, 1, seed=1) / c_img ** 0.5, 0.1 * rn(chan, seed=2)
    w_out, b_out = rn(c_img, chan, 1, 1, seed=3) / chan ** 0.5, 0.1 * rn(c_img, seed=4)
    feat = rn(B, chan, H, W, seed=5)

    def expr_in(img, w, b, sigma):
        return F.conv2d(img * scalings(sigma, sd)[2][:, None, None, None] if pre else img, w, b)

    def expr_out(feat, w, b, img, sigma):
        f = F.conv2d(feat, w, b)
        if not pre:
            return f
        c_skip, c_out, _ = scalings(sigma, sd)
        return f * c_out[:, None, None, None] + img * c_skip[:, None, None, None]
    in64 = expr_in(img.double(), w_in.double(), b_in.double(), sigma.double())
    y = uo.unet_in(g(img), g(w_in), g(b_in), g(sigma) if pre else None, sd)
    within(nchw(y, B, H, W), in64, (expr_in(img, w_in, b_in, sigma).double() - in64).abs().max().item(), f"unet_in {c_img}->{chan} pre={pre}")
    out64 = expr_out(feat.double(), w_out.double(), b_out.double(), img.double(), sigma.double())
    o = uo.unet_out(g(tokens(feat)), g(w_out), g(b_out), (B, c_img, H, W), image=g(img) if pre else None, sigma=g(sigma) if pre else None, sigma_data=sd)
    within(o, out64, (expr_out(feat, w_out, b_out, img, sigma).double() - out64).abs().max().item(), f"unet_out {chan}->{c_img} pre={pre}")


@pytest.mark.parametrize("rows,n_out,k_in,gelu,add", [(3, 64, 9, False, True), (3, 200, 64, True, False), (2, 1154, 256, False, False),
                                                      (5, 64, 100, True, True)], ids=str)
def test_cond_mlp_matches_fp64(KD, rows, n_out, k_in, gelu, add):
    uo = KD.unet_ops
    x, w, b = rn(rows, k_in, seed=n_out), rn(n_out, k_in, seed=k_in) / k_in ** 0.5, 0.2 * rn(n_out, seed=3)
    a = rn(rows, n_out, seed=4) if add else None

    def expr(x, w, b, a):
        y = F.linear(x, w, b)
        y = y if a is None else y + a
        return F.gelu(y) if gelu else y
    y64 = expr(x.double(), w.double(), b.double(), None if a is None else a.double())
    y = uo.cond_mlp(g(x), g(w), g(b), add=None if a is None else g(a), gelu=gelu)
    within(y, y64, (expr(x, w, b, a).double() - y64).abs().max().item(), f"cond_mlp {rows}x{k_in}->{n_out} gelu={gelu} add={add}")
    assert torch.equal(y, uo.cond_mlp(g(x), g(w), g(b), add=None if a is None else g(a), gelu=gelu))


# ---- 5. guard bands: every new kernel, one ragged shape each -------------------------------------------------------------------------------------

def _lib_call(name, *args):
    nat.check(getattr(nat.lib(), name)(*args, stream()), name)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _conv_case(ks, ci, co, hw):
    def make(env):
        B, (H, W) = 2, hw
        x, w, b, r, ref, bound = conv_reference(ks, ci, co, hw, True, True)

        def call(T):
            _lib_call("kd_pack_conv_x3", _p(T["w"]), _p(T["wp"]), co, ci, ks)
            _lib_call("kd_conv2d_x3", _p(T["x"]), ci, _p(T["wp"]), _p(T["b"]), _p(T["r"]), co, _p(T["y"]), co, B, H, W, ci, co, ks)
            return T["y"]

        def tol(got, want):
            err = ((got.cpu().double() - want) .abs() / tokens(bound)).max().item()
            assert err < SPLIT3, f"{err:.3e} of sum|a||w|"
            return err
        return dict(ins={"x": tokens(x), "w": w, "b": b, "r": tokens(r)}, outs={"wp": ((4 * ks * ks * ci * co,), torch.uint8), "y": ((B * H * W, co), F32)},
                    call=call, ref=lambda R: tokens(ref), tol=tol)
    return Case(f"conv2d_x3[k{ks},{ci}->{co},{hw[0]}x{hw[1]}]", "conv2d", "conv_x3.hip", make, mode="split3", kernel="conv2d_x3")


def _adagn_case():
    def make(env):
        chan, hw = 64, (7, 7)
        x, w, b, y64, base = adagn_reference(chan, hw, False, True)
        B = x.shape[0]

        def call(T):
            _lib_call("kd_groupnorm_stats_f32", _p(T["x"]), chan, _p(T["st"]), B, hw[0] * hw[1], chan, chan // 32, C.c_float(1e-5))
            _lib_call("kd_adagn_apply_f32", _p(T["x"]), chan, _p(T["st"]), _p(T["wb"]), 2 * chan, _p(T["y"]), chan, B, hw[0] * hw[1], chan, chan // 32, 1)
            return T["y"], T["st"]
        return dict(ins={"x": tokens(x), "wb": torch.cat([w, b], 1)}, outs={"st": ((B, chan // 32, 4), F32), "y": ((B * 49, chan), F32)}, call=call,
                    ref=lambda R: (tokens(y64), None), tol=[("abs", 4 * base), None])
    return Case("adagn[64,7x7]", "adagn_apply", "unet_f32.hip", make, kernel="adagn_apply_f32")


def _resample_case(up):
    def make(env):
        B, chan, H, W = 2, 64, 6, 2
        x = rn(B, chan, H, W, seed=77)
        fn, kern = (ur.upsample, K_UP) if up else (ur.downsample, K_DOWN)
        y64 = fn(x.double(), kern)
        base = (fn(x, kern).double() - y64).abs().max().item()
        rows = B * (4 * H * W if up else H * W // 4)

        def call(T):
            _lib_call("kd_up2_f32" if up else "kd_down2_f32", _p(T["x"]), chan, _p(T["y"]), chan, B, H, W, chan)
            return T["y"]
        return dict(ins={"x": tokens(x)}, outs={"y": ((rows, chan), F32)}, call=call, ref=lambda R: tokens(y64), tol=("abs", 4 * base))
    return Case("up2[6x2]" if up else "down2[6x2]", "up2" if up else "down2", "unet_f32.hip", make, kernel="up2_f32" if up else "down2_f32")


def _proj_case():
    def make(env):
        B, c_img, chan, H, W, sd = 3, 3, 64, 5, 3, 0.5
        img, sigma = rn(B, c_img, H, W, seed=9), torch.tensor([0.02, 1.5, 70.0])
        w_in, b_in, w_out, b_out = rn(chan, c_img, seed=1), 0.1 * rn(chan, seed=2), rn(c_img, chan, seed=3) / 8, 0.1 * rn(c_img, seed=4)

        def expr(img, sigma, w_in, b_in, w_out, b_out):
            c_skip, c_out, c_in = (t[:, None, None, None] for t in scalings(sigma, sd))
            t = F.conv2d(img * c_in, w_in[:, :, None, None], b_in)
            return F.conv2d(t, w_out[:, :, None, None], b_out) * c_out + img * c_skip, t
        ins = {"img": img, "sigma": sigma, "w_in": w_in, "b_in": b_in, "w_out": w_out, "b_out": b_out}
        o64, t64 = expr(*(v.double() for v in ins.values()))
        o32, t32 = expr(*ins.values())

        def call(T):
            _lib_call("kd_unet_in_f32", _p(T["img"]), _p(T["w_in"]), _p(T["b_in"]), _p(T["sigma"]), C.c_float(sd), _p(T["t"]), chan, B, H * W, c_img, chan)
            _lib_call("kd_unet_out_f32", _p(T["t"]), chan, _p(T["w_out"]), _p(T["b_out"]), _p(T["img"]), _p(T["sigma"]), C.c_float(sd), _p(T["o"]), B, H * W, c_img, chan)
            return T["o"], T["t"]
        return dict(ins=ins, outs={"t": ((B * H * W, chan), F32), "o": ((B, c_img, H, W), F32)}, call=call, ref=lambda R: (o64, tokens(t64)),
                    tol=[("abs", 4 * (o32.double() - o64).abs().max().item()), ("abs", 4 * (t32.double() - t64).abs().max().item())])
    return Case("unet_in_out[3,64,5x3]", "unet_in", "unet_f32.hip", make, kernel="unet_in_f32")


def _mlp_case():
    def make(env):
        rows, n_out, k_in = 3, 70, 33
        x, w, b, a = rn(rows, k_in, seed=1), rn(n_out, k_in, seed=2) / 6, 0.2 * rn(n_out, seed=3), rn(rows, n_out, seed=4)
        y64 = F.gelu(F.linear(x.double(), w.double(), b.double()) + a.double())
        base = (F.gelu(F.linear(x, w, b) + a).double() - y64).abs().max().item()

        def call(T):
            _lib_call("kd_cond_mlp_f32", _p(T["x"]), _p(T["w"]), _p(T["b"]), _p(T["a"]), _p(T["y"]), rows, n_out, k_in, 1)
            return T["y"]
        return dict(ins={"x": x, "w": w, "b": b, "a": a}, outs={"y": ((rows, n_out), F32)}, call=call, ref=lambda R: y64, tol=("abs", 4 * base))
    return Case("cond_mlp[3x33->70]", "cond_mlp", "unet_f32.hip", make, kernel="cond_mlp_f32")


GUARD_CASES = [_conv_case(3, 128, 128, (5, 9)), _conv_case(3, 64, 64, (7, 7)), _conv_case(1, 128, 384, (5, 9)), _adagn_case(), _resample_case(False),
               _resample_case(True), _proj_case(), _mlp_case()]


@pytest.mark.parametrize("c", GUARD_CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")


# ---- 6. the model -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def built(name):
    import k_diffusion_amd as K
    cfg = K.config.load_config(ur.CONFIGS[name])
    model = K.config.make_model(cfg).eval().requires_grad_(False)
    sd = K.synth.synth_state_dict(model.state_dict(), seed=ur.SEED)
    model.load_state_dict(sd)
    return cfg, model.to(DEV), sd


@functools.lru_cache(maxsize=None)
def forward_reference(name):
    """(inputs, fp64 restatement, the reference's recorded fp32 output): computed once."""
    from safetensors.torch import load_file
    _, _, sd = built(name)
    x, sigma, aug = ur.inputs(name)
    return (x, sigma, aug), ur.forward(sd, x, sigma, aug_cond=aug), load_file(os.path.join(REPO, "tests", "golden", "unet_v1.safetensors"))[name + ".out"]


def rel(a, b):
    return ((a.detach().cpu().double() - b.double()).abs().max() / b.double().abs().max()).item()


def _kw(aug):
    return {} if aug is None else {"aug_cond": g(aug)}


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_matches_restatement_and_golden(KD, name, monkeypatch):
    _, model, _ = built(name)
    (x, sigma, aug), ref64, gold = forward_reference(name)
    with torch.no_grad():
        y = model(g(x), g(sigma), **_kw(aug))
        again = model(g(x), g(sigma), **_kw(aug))
    e64, eg = rel(y, ref64), rel(y, gold)
    print(f"{name}: {e64:.3e} from the fp64 restatement (5e-4), {eg:.3e} from the reference's fp32 output (1e-3)")
    assert y.shape == x.shape and e64 < 5e-4 and eg < 1e-3
    assert torch.equal(y, again), "a second forward gives other bits"
    # fp32-grade whatever KDIFF_GEMM says
    monkeypatch.setenv("KDIFF_GEMM", "bf16")
    with torch.no_grad():
        yb = model(g(x), g(sigma), **_kw(aug))
    assert torch.equal(y, yb)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_denoiser_fuses_the_preconditioning(KD, name):
    cfg, model, _ = built(name)
    (x, sigma, aug), _, _ = forward_reference(name)
    sd = cfg["model"]["sigma_data"]
    with torch.no_grad():
        fused = KD.Denoiser(model, sd)(g(x), g(sigma), **_kw(aug))
        f = model(KD.ops.precond_in(g(x), g(sigma), sd), g(sigma), **_kw(aug))
        unfused = KD.ops.precond_out(f.contiguous(), g(x), g(sigma), sd)
    err = rel(fused, unfused.cpu())
    print(f"{name}: fused against unfused preconditioning {err:.3e} (1e-6)")
    assert err < 1e-6
    den = ur.denoiser(built(name)[2], sd)
    assert rel(fused, den(x, sigma, **({} if aug is None else {"aug_cond": aug}))) < 5e-4


def test_sampler_trajectory_matches_restatement(KD):
    from oracle import solvers
    cfg, model, sd = built("unet_a")
    mc = cfg["model"]
    x = torch.stack([KD.synth.synth_noise((3, 12, 20), 3, i, mc["sigma_max"]) for i in range(2)])
    sig = KD.sampling.get_sigmas_karras(6, mc["sigma_min"], mc["sigma_max"], device=DEV)
    with torch.no_grad():
        got = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), g(x), sig, disable=True)
        again = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), g(x), sig, disable=True)
    den = solvers.denoiser(lambda xx, s, **kw: ur.forward(sd, xx, s, **kw), mc["sigma_data"])
    ref = solvers.sample_dpmpp_2m(den, x.double(), sig.cpu().double())
    err = rel(got, ref)
    print(f"unet_a: 6-step DPM++(2M) against the fp64 restatement {err:.3e} (1e-3)")
    assert err < 1e-3 and torch.equal(got, again)


def test_changed_weights_are_noticed(KD):
    """Plans, packed conv images and the AdaGN mapper table follow the weights: after every kind of change the model computes what a fresh
    model with the same weights computes, bit for bit; an unchanged model plans once."""
    cfg, _, sd = built("unet_a")
    (x, sigma, aug), _, _ = forward_reference("unet_a")

    def fresh(state):
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(state)
        return model.to(DEV)

    def run(model):
        with torch.no_grad():
            return model(g(x), g(sigma), **_kw(aug))
    model = fresh(sd)
    inner = getattr(model, "inner_model", model)
    outs = [run(model)]
    n = len(inner._plans)
    assert n == 1 and torch.equal(run(model), outs[0]) and len(inner._plans) == n

    def changed(what):
        outs.append(run(model))
        assert torch.equal(outs[-1], run(fresh(model.state_dict()))), f"{what}: not what a fresh model with these weights computes"
        assert not torch.equal(outs[-1], outs[-2]), f"{what}: the output did not move"
        assert len(inner._plans) == n
    model.load_state_dict(KD.synth.synth_state_dict(model.state_dict(), seed=ur.SEED + 1))
    changed("load_state_dict")
    conv = inner.u_net.d_blocks[0][1].main[2]
    with torch.no_grad():
        conv.weight.mul_(1.5)
    changed("in-place mul_ of a conv weight")
    conv.weight = torch.nn.Parameter(conv.weight.detach() * 0.5, requires_grad=False)
    changed("a parameter assigned anew")


def test_plans_are_dropped_least_recently_used_first(KD):
    _, model, _ = built("unet_a")
    inner = getattr(model, "inner_model", model)
    bound = KD.models.image_v1.MAX_PLANS
    assert bound == 8
    (x, sigma, aug), _, _ = forward_reference("unet_a")
    x, sigma, aug = (None if t is None else g(t).repeat(4, *[1] * (t.dim() - 1)) for t in (x, sigma, aug))

    def run(b):
        with torch.no_grad():
            return model(x[:b], sigma[:b], **({} if aug is None else {"aug_cond": aug[:b]}))
    first = run(3).clone()
    for b in range(1, 11):
        run(b)
        assert len(inner._plans) <= bound
    assert [k[0] for k in inner._plans] == list(range(3, 11))          # the most recent eight, oldest first
    assert torch.equal(run(3), first)                                  # a hit: batch 3 is the most recently used now
    run(1)
    assert [k[0] for k in inner._plans] == [5, 6, 7, 8, 9, 10, 3, 1]
    assert torch.equal(run(4), run(4)) and len(inner._plans) == bound  # a dropped shape is planned again


def test_model_refusals_on_the_device(KD):
    _, model, _ = built("unet_b")
    (x, sigma, _), _, _ = forward_reference("unet_b")
    with torch.no_grad():
        with pytest.raises(ValueError, match="input size 28x30"):
            model(g(torch.zeros(2, 1, 28, 30)), g(sigma))
        with pytest.raises(ValueError, match="mapping_cond"):
            model(g(x), g(sigma), mapping_cond=g(torch.zeros(2, 9)))
        with pytest.raises(ValueError, match="input is"):
            model(g(torch.zeros(2, 3, 28, 28)), g(sigma))
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model(g(x).requires_grad_(True), g(sigma))


def test_sample_py_writes_images(KD, tmp_path):
    """sample.py end to end on an image_v1 config, in process as tests/test_model_gpu.py runs it: --random-weights, then --checkpoint with a
    safetensors file in the reference's layout that carries the config in its metadata."""
    import sample
    from PIL import Image
    from safetensors.torch import save_file
    cfg = json.loads(json.dumps(ur.UNET_B))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    out = sample.main(["--config", str(tmp_path / "config.json"), "--random-weights", "-n", "3", "--batch-size", "2", "--steps", "4", "--seed", "5",
                       "--prefix", str(tmp_path / "out")])
    assert tuple(out.shape) == (3, 1, 28, 28) and bool(torch.isfinite(out).all())
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".png"))
    assert files == ["out_00000.png", "out_00001.png", "out_00002.png"]
    assert Image.open(tmp_path / files[0]).size == (28, 28)
    save_file({k: v.contiguous() for k, v in built("unet_b")[2].items()}, str(tmp_path / "model.safetensors"), metadata={"config": json.dumps(cfg)})
    out = sample.main(["--checkpoint", str(tmp_path / "model.safetensors"), "-n", "2", "--batch-size", "2", "--steps", "4", "--seed", "5",
                       "--prefix", str(tmp_path / "ckpt")])
    assert tuple(out.shape) == (2, 1, 28, 28)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("ckpt_")) == ["ckpt_00000.png", "ckpt_00001.png"]

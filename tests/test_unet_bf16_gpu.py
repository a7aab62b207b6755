"""bf16 convolution arithmetic of the image_v1 U-Net's sampling forward on the MI355X: the kernel ``kd_conv2d_bf16`` (csrc/conv_bf16.hip;
``unet_ops.conv2d(bf16=True)``), ``set_conv_arithmetic("bf16")`` on the bare and the wrapped model, and ``sample.py --unet-arithmetic bf16``.

Bounds.
* kernel: truth is the fp64 ``F.conv2d`` of the operands rounded by ``.bfloat16()`` on the CPU (plus bias and residual); the error is taken per
  element relative to sum |a^||w^|; the yardstick is torch's fp32 CPU convolution of the same rounded operands under the same measure;
  ``err <= max(4 yardstick, 2^-21)`` -- ``rounded_reference``'s idiom of tests/test_unet_mixed_gpu.py: with both operands rounded beforehand the
  only error source left is the order of the fp32 accumulation.  ``kd_conv2d_x3`` on the UNROUNDED operands must miss that bound: the test
  tells the two arithmetics apart.
* scaling: bit for bit (tests/scaling.py): bf16 rounding commutes with a power of two while nothing goes subnormal.
* wiring, other passes: bit for bit.
* model: the max-norm distance of the bf16 forward from the reference's recorded fp32 output (tests/golden/unet_v1.safetensors) is at most 2 x
  the reference's own distance under ``torch.autocast('cpu', dtype=torch.bfloat16)`` (tests/golden/unet_bf16.safetensors): both are the
  largest of many independent bf16 roundings through a deep network, and single draws of such a maximum moved by about 20 % between seeds.
"""
import functools
import json
import os

import pytest
import torch
from torch.nn import functional as F

from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.scaling import Relation, factors, run_relation
from tests.guard import Case
from tests.test_unet_gpu import CONV_CASES, DEV, conv_reference, g, nchw, rn, tokens
from tests.test_unet_train_gpu import grads_of, hip_loss, profiled, trainable

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -21
# tests/test_unet_gpu.CONV_CASES (B = 2; 7x7, 8x8, 5x9, 14x14; 64->128, 384->64, 128->128 at ks 3, 128->384 and 64->192 at ks 1; bias, residual and
# wide strides rotating) plus a 2 x 2 image, smaller than a patch, for each kernel size and each N tile
CASES = CONV_CASES + [(3, 64, 128, (2, 2), True, True, False), (1, 64, 192, (2, 2), True, False, True)]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rounded_reference(ks, ci, co, hw, bias, residual):
    """(x, w, b, r, truth, sum |a^||w^|, yardstick): the UNROUNDED operands of ``conv_reference``; truth = fp64 conv2d of the operands rounded by
    ``.bfloat16()``, + bias + residual; yardstick = the largest error, per element relative to sum |a^||w^|, of the same expression in fp32 on the
    CPU."""
    x, w, b, r, _, _ = conv_reference(ks, ci, co, hw, bias, residual)
    xb, wb = x.bfloat16(), w.bfloat16()
    truth = F.conv2d(xb.double(), wb.double(), None if b is None else b.double(), padding=ks // 2)
    yard = F.conv2d(xb.float(), wb.float(), b, padding=ks // 2)
    if r is not None:
        truth, yard = truth + r.double(), yard + r
    scale = F.conv2d(xb.double().abs(), wb.double().abs(), padding=ks // 2)
    assert float(scale.min()) > 0
    return x, w, b, r, truth, scale, ((yard.double() - truth).abs() / scale).max().item()


@pytest.mark.parametrize("ks,ci,co,hw,bias,residual,wide", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv_bf16_error_is_the_accumulation_order(KD, ks, ci, co, hw, bias, residual, wide):
    """Measured (error / yardstick, MI355X): see DESIGN.md section 8."""
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    x, w, b, r, truth, scale, e_yard = rounded_reference(ks, ci, co, hw, bias, residual)
    bound = max(4 * e_yard, FLOOR)
    rows = B * H * W
    if wide:                 # the concat halves: x is the right half of a [rows, 2 ci] buffer, y the left half of a [rows, co + 64] one
        xbuf = torch.full((rows, 2 * ci), float("nan"), device=DEV)
        xbuf[:, ci:] = g(tokens(x))
        xt = xbuf[:, ci:]
        ybuf = torch.full((rows, co + 64), -7.0, device=DEV)
        out = ybuf[:, :co]
    else:
        xt, out, ybuf = g(tokens(x)), None, None
    wt, bt, rt = g(w), None if b is None else g(b), None if r is None else g(tokens(r))
    y, names = profiled(KD._native, lambda: uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt, out=out, bf16=True))
    err = ((nchw(y.cpu().double(), B, H, W) - truth).abs() / scale).max().item()
    split = uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt)
    e_split = ((nchw(split.cpu().double(), B, H, W) - truth).abs() / scale).max().item()
    print(f"conv bf16 k{ks} {ci}->{co} {H}x{W} bias={bias} res={residual} wide={wide}: error {err:.3e} of sum|a^||w^| = "
          f"{err / max(e_yard, 1e-300):.2f} x the yardstick {e_yard:.3e} (bound {bound:.3e}); the split kernel on the unrounded operands "
          f"{e_split:.3e} = {e_split / bound:.0f} x the bound; {names}")
    assert y.shape == (rows, co)
    assert err <= bound
    assert not e_split <= bound, "the bound cannot tell bf16 operands from unrounded ones"
    tile = 128 if co % 128 == 0 else 64
    assert [nm.split(" ")[0] for nm in names if nm.startswith("conv2d")] == [f"conv2d_bf16<k{ks},n{tile}>"], names
    if wide:
        assert bool((ybuf[:, co:] == -7.0).all()), "the columns beside the output range were written"
    assert torch.equal(y, uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt, bf16=True)), "a repeat gives other bits"


def test_conv_bf16_refuses_what_conv2d_x3_refuses(KD):
    uo = KD.unet_ops
    with pytest.raises(RuntimeError, match="kd_conv2d_bf16.*multiples of 64"):
        uo.conv2d(g(rn(8, 32)), g(rn(64, 32, 1, 1)), 2, 2, 2, bf16=True)
    with pytest.raises(RuntimeError, match="kernel size"):             # (the pack kernel refuses it first)
        uo.conv2d(g(rn(8, 64)), g(rn(64, 64, 5, 5)), 2, 2, 2, bf16=True)
    with pytest.raises(RuntimeError, match="kd_conv2d_bf16.*kernel size"):         # ... and the entry point itself, handed a packed image
        uo.conv2d(g(rn(8, 64)), g(rn(64, 64, 5, 5)), 2, 2, 2, packed=uo.pack_conv(g(rn(64, 64, 3, 3))), bf16=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.conv2d(rn(8, 64), g(rn(64, 64, 1, 1)), 2, 2, 2, bf16=True)
    x, w = g(rn(8, 64)), g(rn(64, 64, 1, 1))
    with pytest.raises(ValueError, match="bias_batch"):
        uo.conv2d(x, w, 2, 2, 2, bias=g(rn(64)), bias_batch=1, bf16=True)
    with pytest.raises(ValueError, match="chan_scale"):
        uo.conv2d(x, w, 2, 2, 2, chan_scale=g(rn(2, 64)), bf16=True)


def test_conv_bf16_rounds_to_nearest_even(KD):
    """A one-hot weight of 1 copies one input channel to one output channel, rounded: ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), near-ties
    (1 + 2^-8 + 2^-20 -> 1 + 2^-7) and their negatives come out as ``x.bfloat16()``, bit for bit -- nearest even, and no lo part."""
    uo = KD.unet_ops
    B, H, W, ci, co = 2, 9, 11, 128, 64
    vals = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])
    vals = torch.cat([vals, -vals])
    x = vals[(torch.arange(B * H * W * ci) * 7 // 3) % 6].reshape(B * H * W, ci)
    for ks in (3, 1):
        w = torch.zeros(co, ci, ks, ks)
        w[13, 37, ks // 2, ks // 2] = 1.0
        y = uo.conv2d(g(x), g(w), B, H, W, bf16=True).cpu()
        want = torch.zeros(B * H * W, co)
        want[:, 13] = x[:, 37].bfloat16().float()
        assert torch.equal(y, want) and not torch.equal(want[:, 13], x[:, 37])


# ---- 2. neighbour isolation ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ks,hw", [(3, (7, 7)), (3, (8, 8)), (1, (5, 9))])
def test_conv_bf16_never_reads_the_neighbouring_sample(KD, ks, hw):
    uo = KD.unet_ops
    B, (H, W) = 2, hw
    x, w, *_ = conv_reference(ks, 128, 128 if ks == 3 else 384, hw, False, False)
    xt = g(tokens(x)).view(B, H * W, -1)
    base = uo.conv2d(xt.view(B * H * W, -1), g(w), B, H, W, bf16=True).view(B, H * W, -1)
    for other, fill in ((0, 1e30), (1, float("nan"))):
        x2 = xt.clone()
        x2[other] = fill
        y2 = uo.conv2d(x2.view(B * H * W, -1), g(w), B, H, W, bf16=True).view(B, H * W, -1)
        assert torch.equal(y2[1 - other], base[1 - other]), f"sample {1 - other} changed when sample {other} was filled with {fill}"


# ---- 3. power-of-two scaling -----------------------------------------------------------------------------------------------------------------------

def _scaling_case(ks, ci, co, hw):
    def make(env):
        B, (H, W) = 2, hw
        x, w, b, r, *_ = conv_reference(ks, ci, co, hw, True, True)
        return dict(ins={"x": tokens(x), "w": w, "b": b, "r": tokens(r)},
                    call=lambda T: env.unet_ops.conv2d(T["x"], T["w"], B, H, W, bias=T["b"], residual=T["r"], bf16=True))
    return Case(f"conv2d_bf16[k{ks},{ci}->{co},{hw[0]}x{hw[1]}]", "conv2d", "conv_bf16.hip", make, kernel="conv2d_bf16")


def _per_sample(f, t):
    return f.repeat_interleave(t.shape[0] // f.numel())[:, None]


def _sample(ins, outs):
    """x and the residual scaled per sample (the bias zeroed in both calls): y scales per sample"""
    f = factors(2, 1)
    return {"x": _per_sample(f, ins["x"]), "r": _per_sample(f, ins["r"])}, [_per_sample(f, ins["x"])]


def _c_out(ins, outs):
    """w, the bias and the residual scaled per output channel: y scales per output channel"""
    f = factors(ins["w"].shape[0], 2)
    return {"w": f.view(-1, 1, 1, 1), "b": f, "r": f[None, :]}, [f[None, :]]


SCALING_CASES = [_scaling_case(3, 64, 128, (7, 7)), _scaling_case(1, 64, 192, (5, 9))]


@pytest.mark.parametrize("c", SCALING_CASES, ids=repr)
def test_conv_bf16_commutes_with_power_of_two_scaling(KD, c):
    """Exponents in [-20, 20] on operands within [1e-7, 1e4]: tests/scaling.py asserts that every scaled input stays inside [2^-60, 2^60] and that
    no result is flushed, so nothing is subnormal in fp32 or in bf16 (the same exponent range) and rounding commutes with the factors."""
    spec = None
    for relation in (Relation("c_out", _c_out), Relation("sample", _sample, zero=("b",))):
        (spec, _), names = profiled(KD._native, lambda: run_relation(c, relation, env=KD, device=DEV, spec=spec))
        served = [nm.split("<")[0] for nm in names if nm.startswith("conv2d")]
        assert served == ["conv2d_bf16", "conv2d_bf16"], names           # the baseline call and the scaled call
        print(f"{c.name} / {relation.name}: same bits as the scaled baseline")


# ---- 4. the model: wiring -------------------------------------------------------------------------------------------------------------------------

def fresh(KD, name):
    import k_diffusion_amd as K
    cfg = K.config.load_config(ur.CONFIGS[name])
    model = K.config.make_model(cfg).eval().requires_grad_(False)
    model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=ur.SEED))
    return cfg, model.to(DEV)


def _inputs(name):
    x, sigma, aug = ur.inputs(name)
    return g(x), g(sigma), ({} if aug is None else {"aug_cond": g(aug)})


def _count(names, prefix):
    return sum(nm.startswith(prefix) for nm in names)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_the_setting_is_conv2d_with_bf16_and_nothing_else(KD, name, monkeypatch):
    _, model = fresh(KD, name)
    x, sigma, kw = _inputs(name)
    with torch.no_grad():                                              # (each plan is built, and its weights packed, before the profiled call)
        first = model(x, sigma, **kw)
        y0, names0 = profiled(KD._native, lambda: model(x, sigma, **kw))
        assert torch.equal(first, y0)
        assert model.set_conv_arithmetic("bf16") is model
        again = model(x, sigma, **kw)
        y1, names1 = profiled(KD._native, lambda: model(x, sigma, **kw))
    n_x3, n_bf16 = _count(names0, "conv2d_x3"), _count(names1, "conv2d_bf16")
    print(f"{name}: {n_x3} conv2d_x3 launches of {len(names0)} in the fp32-grade forward, {n_bf16} conv2d_bf16 of {len(names1)} in the bf16 forward")
    assert n_x3 > 0 and _count(names0, "conv2d_bf16") == 0
    assert _count(names1, "conv2d_x3") == 0 and n_bf16 == n_x3 and len(names1) == len(names0)
    strip = [nm.split("<")[0].replace("conv2d_bf16", "conv2d_x3") if nm.startswith("conv2d") else nm for nm in names1]
    assert strip == [nm.split("<")[0] if nm.startswith("conv2d") else nm for nm in names0], "another launch moved too"
    assert torch.equal(y1, again) and not torch.equal(y1, y0)
    # an unset model whose every unet_ops.conv2d is handed bf16=True computes the same bits
    _, other = fresh(KD, name)
    plain = KD.unet_ops.conv2d
    monkeypatch.setattr(KD.unet_ops, "conv2d", lambda *a, **k: plain(*a, **dict(k, bf16=True)))
    with torch.no_grad():
        y2 = other(x, sigma, **kw)
    monkeypatch.undo()
    assert getattr(other, "inner_model", other).conv_arithmetic is None
    assert torch.equal(y1, y2), "set_conv_arithmetic('bf16') is not conv2d(bf16=True) at every site"
    # switched off again: the fp32-grade forward's bits
    assert model.set_conv_arithmetic(None) is model
    with torch.no_grad():
        assert torch.equal(model(x, sigma, **kw), y0)
    # the fused preconditioning takes the same plan
    sd = ur.CONFIGS[name]["model"]["sigma_data"]
    with torch.no_grad():
        d0 = KD.Denoiser(model, sd)(x, sigma, **kw)
        d1, names_d = profiled(KD._native, lambda: KD.Denoiser(model.set_conv_arithmetic("bf16"), sd)(x, sigma, **kw))
    assert _count(names_d, "conv2d_bf16") == n_x3 and _count(names_d, "conv2d_x3") == 0 and not torch.equal(d0, d1)


# ---- 5. the other passes keep their bits ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_the_dual_and_reverse_passes_keep_their_bits(KD, name):
    _, model = fresh(KD, name)
    x, sigma, kw = _inputs(name)
    v, u = g(rn(*x.shape, seed=23)), g(rn(*x.shape, seed=29))
    runs = []
    for arithmetic in (None, "bf16"):
        model.set_conv_arithmetic(arithmetic)
        with torch.no_grad():
            f, fd = model.forward_jvp(x, sigma, v, **kw)
        (out, pull), names = profiled(KD._native, lambda: model.forward_vjp(x, sigma, **kw))
        runs.append((f, fd, out, pull(u)))
        assert _count(names, "conv2d_bf16") == 0, names
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_the_training_loss_keeps_its_bits(KD, name):
    runs = []
    for arithmetic in (None, "bf16"):
        model = trainable(KD, name)
        model.set_conv_arithmetic(arithmetic)
        losses, names = profiled(KD._native, lambda: hip_loss(KD, model, name, "karras"))
        losses.mean().backward()
        torch.cuda.synchronize()
        runs.append((losses.detach().clone(), {k: v.clone() for k, v in grads_of(model).items()}))
        assert _count(names, "conv2d_bf16") == 0, names
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1) and sorted(g0) == sorted(g1) and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ---- 6. the end-to-end envelope, against the reference's own autocast error -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_error_within_twice_the_references_autocast_error(KD, name):
    """Measured (MI355X): see DESIGN.md section 8."""
    from safetensors.torch import load_file
    gold = load_file(os.path.join(REPO, "tests", "golden", "unet_v1.safetensors"))[name + ".out"]
    auto = load_file(os.path.join(REPO, "tests", "golden", "unet_bf16.safetensors"))[name + ".out_autocast_bf16"]
    _, model = fresh(KD, name)
    x, sigma, kw = _inputs(name)
    with torch.no_grad():
        y0 = model(x, sigma, **kw)
        y1 = model.set_conv_arithmetic("bf16")(x, sigma, **kw)
    top = gold.double().abs().max().item()
    e_ref = (auto.double() - gold.double()).abs().max().item()
    e_ours = (y1.cpu().double() - gold.double()).abs().max().item()
    e_fp32 = (y0.cpu().double() - gold.double()).abs().max().item()
    print(f"{name}: bf16 forward {e_ours:.3e} ({e_ours / top:.3e} relative) from the reference's fp32 output; the reference under autocast(bf16) "
          f"{e_ref:.3e} ({e_ref / top:.3e}); ratio {e_ours / e_ref:.3f} (bound 2); the fp32-grade forward {e_fp32 / top:.3e}")
    assert e_ref > 0 and y1.shape == gold.shape
    assert e_ours <= 2 * e_ref


# ---- 7. sampling -------------------------------------------------------------------------------------------------------------------------------------

def test_a_sampler_run_in_the_mode_finishes_finite(KD):
    cfg, model = fresh(KD, "unet_a")
    mc = cfg["model"]
    x = torch.stack([KD.synth.synth_noise((3, 12, 20), 3, i, mc["sigma_max"]) for i in range(2)])
    sig = KD.sampling.get_sigmas_karras(6, mc["sigma_min"], mc["sigma_max"], device=DEV)
    with torch.no_grad():
        ref = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), g(x), sig, disable=True)
        model.set_conv_arithmetic("bf16")
        got = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), g(x), sig, disable=True)
        again = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), g(x), sig, disable=True)
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"unet_a: 6-step DPM++(2M) in the bf16 mode, {err:.3e} from the fp32-grade trajectory")
    assert got.shape == x.shape and bool(torch.isfinite(got).all()) and torch.equal(got, again) and not torch.equal(got, ref)


def test_sample_py_writes_images_in_the_mode(KD, tmp_path):
    import sample
    from PIL import Image
    cfg = json.loads(json.dumps(ur.UNET_B))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    common = ["--config", str(tmp_path / "config.json"), "--random-weights", "-n", "3", "--batch-size", "2", "--steps", "4", "--seed", "5"]
    out = sample.main([*common, "--unet-arithmetic", "bf16", "--prefix", str(tmp_path / "out")])
    assert tuple(out.shape) == (3, 1, 28, 28) and bool(torch.isfinite(out).all())
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".png"))
    assert files == ["out_00000.png", "out_00001.png", "out_00002.png"]
    assert Image.open(tmp_path / files[0]).size == (28, 28)
    plain = sample.main([*common, "--no-png", "--prefix", str(tmp_path / "plain")])
    assert not torch.equal(out, plain), "the flag changed nothing"

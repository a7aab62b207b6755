"""Dropout in the image_v1 U-Net's training loss on the MI355X: the five entry points of include/kdiff_unet_drop.h against the numpy statement of
the mask contract (tests/unet_drop_ref.py) and fp64 torch, ``Denoiser.loss`` with ``backward()`` in training mode after ``enable_dropout()``
against fp64 autograd over the masked restatement with the SAME Philox masks, and the behaviour around it (seeds, eval, frozen subsets,
retained graphs, which launches name the new kernels).  tests/test_unet_drop_cpu.py ties the restatement to the REAL reference.

Bounds.
* masks and ``kd_chan_scale_f32``: bit for bit.
* ``kd_conv2d_x3_drop``: dropped channels are the residual (or 0) exactly; kept ones meet tests/test_unet_gpu.py's split-bf16x3 bound,
  |got - ref| / (scale * sum |a| |w|) < 2^-14 -- the factor multiplies the sum and its error alike, and adds one fp32 rounding (2^-24).
* attention with dropout: the bounds of the existing tests of the fp32 kernels it is written after -- forward 2e-5 of the largest output
  (tests/test_ops_gpu.py::test_attn_global_sizes for the fp32 arithmetic, on its operands), reverse 1e-5 per q / k / v part
  (tests/test_vjp_gpu.py::test_attn_global_vjp, on its operands).  A mask is an exact factor: one more multiply per term.
* model: tests/test_unet_train_gpu.py's gates for the dropout-free loss, unchanged: losses within 1e-5 relative of fp64 autograd, every
  parameter gradient within 5e-4 (max-abs relative per tensor).

The seed of the model-level tests.  The masks are part of the case, and a case can be ill-conditioned: unet_b has ONE image channel, so the
gradient of ``proj_out.bias`` is a single number, the sum of 2 (F - target) / N over all pixels, and under some keys that sum nearly cancels.
Seed 20 (key 4944179303255885687) gives 8.5e-4 where other keys give 0.2 .. 0.9: there the restatement's own fp32 run is 6.5e-6 from its fp64
run (elsewhere about 1e-6), and the kernels missed the gate at that one parameter with 5.6e-4 while every other gradient of that run was within
2e-5.  The gate is 500 x the reference's usual fp32 error; a case qualifies if the reference's OWN fp32 error on it -- torch on the CPU, no
kernel involved -- leaves at least 100 x of that headroom: fp32 restatement within 5e-6 of fp64 on every parameter gradient.  SEED is the
smallest seed whose key qualifies at both configs and all three weightings (seeds 0 .. 11 measured: 6, 8 and 11 do not); the test asserts the
condition beside the one on the masks, so a seed that stops qualifying says so instead of blaming a kernel.
"""
import functools

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from oracle import hdit
from tests import unet_drop_ref as dr
from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.test_unet_gpu import DEV, SPLIT3, _lib_call, _p, g, nchw, rel, rn, tokens
from tests.test_unet_train_gpu import grads_of, profiled, worst

pytestmark = pytest.mark.gpu
KEYS = (0x1234_5678_9ABC_DEF0, -7)
ATTN_FWD_BOUND = 2e-5
ATTN_VJP_BOUND = 1e-5
DROP_KERNELS = ("chan_mask_f32", "chan_scale_f32", "conv2d_x3_drop", "attn_global_drop")
SEED = 0
CASE_CONDITION = 5e-6          # the fp32 restatement against the fp64 one, worst parameter gradient: see the module docstring


def key_of(k):
    return torch.tensor([k], dtype=torch.int64, device=DEV)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def factors(keep, p):
    """float32 factors (0 or scale) of numpy keep flags."""
    return np.where(keep, dr.scale_of(p), np.float32(0.0)).astype(np.float32)


# ---- 1. the channel table ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.05, 0.5])
@pytest.mark.parametrize("key", KEYS)
def test_chan_mask_matches_the_contract(KD, key, p):
    uo = KD.unet_ops
    B = 3
    sites = [(dr.SITE | 4, 64), (dr.SITE | 5, 128), (dr.SITE | 1 << 20, 64)]
    layout, width = uo.chan_layout(sites)
    assert layout == [(sites[0][0], 0, 64), (sites[1][0], 64, 128), (sites[2][0], 192, 64)] and width == 256
    table = torch.full((B, width + 64), -7.0, device=DEV)              # a table wider than the sites: the columns beside stay
    out = uo.chan_mask(key_of(key), layout, B, p, out=table)
    want = np.concatenate([factors(dr.chan_keep(key, site, p, B, C), p) for site, C in sites], axis=1)
    assert out is table and np.array_equal(bits(table[:, :width]), want.view(np.uint32))
    assert bool((table[:, width:] == -7.0).all())
    assert torch.equal(uo.chan_mask(key_of(key), layout, B, p), table[:, :width]), "a repeat gives other bits"
    assert set(np.unique(want)) == {np.float32(0.0), dr.scale_of(p)}
    for bad in (0.0, 1.0):
        with pytest.raises(ValueError, match="dropout rate"):
            uo.chan_mask(key_of(key), layout, B, bad)


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_chan_mask_drops_the_expected_fraction(KD, p):
    B, C = 256, 256                                                     # B C = 2^16
    table = KD.unet_ops.chan_mask(key_of(KEYS[0]), [(dr.SITE | 2, 0, C)], B, p)
    assert np.array_equal(bits(table), factors(dr.chan_keep(KEYS[0], dr.SITE | 2, p, B, C), p).view(np.uint32))
    frac = (table == 0).double().mean().item()
    sd = (p * (1 - p) / (B * C)) ** 0.5
    print(f"p = {p}: dropped {frac:.5f}, {abs(frac - p) / sd:.2f} standard deviations off")
    assert abs(frac - p) < 5 * sd


# ---- 2. the convolution's epilogue --------------------------------------------------------------------------------------------------------------------

CONV_SHAPE = dict(B=3, hw=(12, 20), ci=64, co=128)                      # 2 x 3 ragged 8 x 8 patches per sample


@functools.lru_cache(maxsize=None)
def conv_drop_reference(ks, bias, residual):
    B, (H, W), ci, co = CONV_SHAPE["B"], CONV_SHAPE["hw"], CONV_SHAPE["ci"], CONV_SHAPE["co"]
    seed = 300 + 10 * ks + 2 * bias + residual
    x, w = rn(B, ci, H, W, seed=seed), rn(co, ci, ks, ks, seed=seed + 1) / (ks * ci ** 0.5)
    b = rn(co, seed=seed + 2) if bias else None
    r = rn(B, co, H, W, seed=seed + 3) if residual else None
    keep = dr.chan_keep(KEYS[1], dr.SITE | 9, 0.5, B, co)
    m = torch.from_numpy(factors(keep, 0.5))
    conv = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=ks // 2)
    ref = conv * m.double()[:, :, None, None] + (0 if r is None else r.double())
    bound = F.conv2d(x.abs().double(), w.abs().double(), padding=ks // 2) * float(dr.scale_of(0.5))
    return x, w, b, r, keep, m, ref, bound


@pytest.mark.parametrize("residual", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ks", [3, 1])
def test_conv_drop_epilogue(KD, ks, bias, residual):
    uo = KD.unet_ops
    B, (H, W), ci, co = CONV_SHAPE["B"], CONV_SHAPE["hw"], CONV_SHAPE["ci"], CONV_SHAPE["co"]
    x, w, b, r, keep, m, ref, bound = conv_drop_reference(ks, bias, residual)
    assert keep.any(axis=1).all() and not keep.all(axis=1).any(), "every sample needs dropped and kept channels"
    rows = B * H * W
    table = torch.full((B, co + 192), float("nan"), device=DEV)        # the site is a column range of a wider table
    table[:, 64:64 + co] = g(m)
    ybuf = torch.full((rows, co + 64), -7.0, device=DEV)               # y is a column range of a wider buffer
    xt, wt = g(tokens(x)), g(w)
    bt, rt = (None if b is None else g(b)), (None if r is None else g(tokens(r)))
    (y, names) = profiled(KD._native, lambda: uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt, out=ybuf[:, :co], chan_scale=table[:, 64:64 + co]))
    assert any(n.startswith("conv2d_x3_drop<") for n in names), names
    assert bool((ybuf[:, co:] == -7.0).all()), "the columns beside the output range were written"
    got = nchw(y.cpu(), B, H, W)
    dropped = torch.from_numpy(~keep)
    want_dropped = (r if r is not None else torch.zeros_like(got))[dropped]
    assert torch.equal(got[dropped], want_dropped), "a dropped channel is the residual (or 0), exactly"
    kept = torch.from_numpy(keep)
    err = ((got.double() - ref).abs() / bound)[kept].max().item()
    print(f"conv drop k{ks} bias={bias} res={residual}: kept channels {err:.3e} of scale * sum|a||w| (bound {SPLIT3:.3e})")
    assert err < SPLIT3
    assert torch.equal(uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt, chan_scale=table[:, 64:64 + co]), y), "a repeat gives other bits"
    # a null table: kd_conv2d_x3's output bit for bit, and its launch name
    plain = uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt)
    null = torch.empty_like(plain)
    (_, names) = profiled(KD._native, lambda: _lib_call("kd_conv2d_x3_drop", _p(xt), ci, _p(uo.pack_conv(wt)), _p(bt), _p(rt), co if rt is not None else 0,
                                                        None, 0, _p(null), co, B, H, W, ci, co, ks))
    assert torch.equal(null, plain) and all(n.startswith("conv2d_x3<") for n in names), names
    # a table of ones is the plain convolution too (x * 1 is x)
    ones = torch.ones(B, co, device=DEV)
    assert torch.equal(uo.conv2d(xt, wt, B, H, W, bias=bt, residual=rt, chan_scale=ones), plain)


def test_conv_drop_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    x, w = g(rn(2 * 16, 64)), g(rn(64, 64, 3, 3))
    with pytest.raises(ValueError, match="chan_scale"):
        uo.conv2d(x, w, 2, 4, 4, chan_scale=torch.ones(3, 64, device=DEV))
    with pytest.raises(ValueError, match="exclude each other"):
        uo.conv2d(x, w, 2, 4, 4, chan_scale=torch.ones(2, 64, device=DEV), bias_batch=1)
    with pytest.raises(RuntimeError, match="chan_stride"):
        _lib_call("kd_conv2d_x3_drop", _p(x), 64, _p(uo.pack_conv(w)), None, None, 0, _p(x), 32, _p(torch.empty(32, 64, device=DEV)), 64, 2, 4, 4, 64, 64, 3)


# ---- 3. the mask's transpose on a gradient ----------------------------------------------------------------------------------------------------------------

def test_chan_scale_is_the_product(KD):
    uo = KD.unet_ops
    B, H, W, C = 3, 12, 20, 128
    gt = g(rn(B * H * W, C, seed=4))
    table = uo.chan_mask(key_of(KEYS[0]), [(dr.SITE | 3, 64, C)], B, 0.25, out=torch.zeros(B, C + 128, device=DEV))
    m = table[:, 64:64 + C]
    want = (gt.view(B, H * W, C) * m[:, None, :]).view(-1, C)
    assert bool((want == 0).any()) and bool((want != 0).any())
    assert torch.equal(uo.chan_scale(gt, m, B), want)
    # strided in, strided out
    wide = torch.full((B * H * W, 2 * C), float("nan"), device=DEV)
    wide[:, C:] = gt
    obuf = torch.full((B * H * W, C + 64), -7.0, device=DEV)
    out = uo.chan_scale(wide[:, C:], m, B, out=obuf[:, :C])
    assert torch.equal(out, want) and bool((obuf[:, C:] == -7.0).all())
    # in place, on a column range
    assert uo.chan_scale(wide[:, C:], m, B, out=wide[:, C:]).data_ptr() == wide[:, C:].data_ptr()
    assert torch.equal(wide[:, C:], want) and bool(torch.isnan(wide[:, :C]).all())
    with pytest.raises(RuntimeError, match="multiples of 4"):
        uo.chan_scale(g(rn(6, 6)), torch.ones(3, 6, device=DEV), 3)
    with pytest.raises(ValueError, match="chan_scale"):
        uo.chan_scale(gt, m[:2], B)


# ---- 4. attention with dropout on the probabilities ---------------------------------------------------------------------------------------------------------

ATTN_B, ATTN_NH, ATTN_P, ATTN_SITE = 2, 2, 0.25, dr.SITE | 14
ATTN_T = [49, 64, 80]          # 49: T4 = 52 != T and a ragged last 16-query block; 64: whole blocks; 80: a third 32-key chunk, half full


def pack_qkv(q, k, v):
    """[B, T, nh, 64] x 3 -> [B, T, 3 nh 64]"""
    return torch.stack([q, k, v], dim=2).reshape(q.shape[0], q.shape[1], -1).contiguous()


def attn_drop_expr(qkv, m, nh):
    """softmax(q k^T) with the factors m [B, nh, T, T] on the probabilities, then @ v, in qkv's dtype: [B, T, nh 64]."""
    B, T, _ = qkv.shape
    q, k, v = (t.transpose(1, 2) for t in qkv.view(B, T, 3, nh, 64).unbind(2))
    prob = torch.softmax(q @ k.transpose(2, 3), dim=-1)
    return ((prob * m) @ v).transpose(1, 2).reshape(B, T, nh * 64)


@functools.lru_cache(maxsize=None)
def attn_mask(T, key):
    keep = dr.attn_keep(key, ATTN_SITE, ATTN_P, ATTN_B, ATTN_NH, T)
    return torch.from_numpy(factors(keep, ATTN_P)).double()


@pytest.mark.parametrize("T", ATTN_T)
def test_attn_global_drop_matches_fp64(KD, T):
    uo = KD.unet_ops
    B, nh, key = ATTN_B, ATTN_NH, KEYS[1]
    q, k, v = (rn(B, T, nh, 64, seed=s) * sc for s, sc in ((1, 0.6), (2, 0.6), (3, 1.0)))     # test_attn_global_sizes' operands
    qkv = pack_qkv(q, k, v)
    m = attn_mask(T, key)
    assert bool((m == 0).any(dim=-1).all()) and bool((m != 0).any(dim=-1).all()), "every probability row needs dropped and kept keys"
    ref = attn_drop_expr(qkv.double(), m, nh)
    (y, names) = profiled(KD._native, lambda: uo.attn_global_drop(g(qkv), nh, key_of(key), ATTN_SITE, ATTN_P))
    err = rel(y, ref)
    plain = rel(KD.ops.attn_global(g(qkv), nh), ref)
    print(f"attention with dropout T={T}: {err:.3e} of the largest ({ATTN_FWD_BOUND:.0e}); without the mask {plain:.3e}; {names}")
    assert names == ["attn_global_drop_f32"]
    assert err < ATTN_FWD_BOUND and plain > 100 * ATTN_FWD_BOUND, "the mask must matter"
    assert torch.equal(uo.attn_global_drop(g(qkv), nh, key_of(key), ATTN_SITE, ATTN_P), y), "a repeat gives other bits"
    other = uo.attn_global_drop(g(qkv), nh, key_of(KEYS[0]), ATTN_SITE, ATTN_P)
    assert rel(other, attn_drop_expr(qkv.double(), attn_mask(T, KEYS[0]), nh)) < ATTN_FWD_BOUND and not torch.equal(other, y)
    # a rate of 0 is today's kernel
    (y0, names0) = profiled(KD._native, lambda: uo.attn_global_drop(g(qkv), nh, None, ATTN_SITE, 0.0))
    assert torch.equal(y0, KD.ops.attn_global(g(qkv), nh)) and not any("drop" in n for n in names0)


@pytest.mark.parametrize("T", ATTN_T)
def test_attn_global_drop_vjp_matches_fp64(KD, T):
    uo = KD.unet_ops
    B, nh, key = ATTN_B, ATTN_NH, KEYS[0]
    gen = torch.Generator().manual_seed(10 + T)                         # test_attn_global_vjp's operands: prepared q, k of length sqrt(10)
    q, k, v = (torch.randn(B, 1, T, nh, 64, generator=gen) for _ in range(3))
    q, k = hdit.cosine_sim_scale(q, k, torch.full([nh], 10.0))
    qkv = pack_qkv(q[:, 0], k[:, 0], v[:, 0])
    go = torch.randn(B, T, nh * 64, generator=gen)
    m = attn_mask(T, key)
    x64 = qkv.double().requires_grad_()
    ref, = torch.autograd.grad(attn_drop_expr(x64, m, nh), x64, go.double())
    (out, names) = profiled(KD._native, lambda: uo.attn_global_drop_vjp(g(qkv), g(go), nh, key_of(key), ATTN_SITE, ATTN_P))
    assert names == ["attn_global_drop_vjp_f32"] * 2, names
    plain = KD.ops.attn_global_vjp(g(qkv), g(go), nh)
    for part, what in enumerate("qkv"):                                 # each slot comes from its own sweep
        sl = lambda t: t.reshape(B, T, 3, nh * 64)[:, :, part]
        err, off = rel(sl(out), sl(ref)), rel(sl(plain), sl(ref))
        print(f"attention reverse with dropout T={T} d{what}: {err:.3e} of the largest ({ATTN_VJP_BOUND:.0e}); without the mask {off:.3e}")
        assert err < ATTN_VJP_BOUND and off > 100 * ATTN_VJP_BOUND
    assert torch.equal(uo.attn_global_drop_vjp(g(qkv), g(go), nh, key_of(key), ATTN_SITE, ATTN_P), out), "a repeat gives other bits"
    (g0, names0) = profiled(KD._native, lambda: uo.attn_global_drop_vjp(g(qkv), g(go), nh, None, ATTN_SITE, 0.0))
    assert torch.equal(g0, plain) and not any("drop" in n for n in names0)


# ---- 5. the model: Denoiser.loss and backward() in training mode ------------------------------------------------------------------------------------------

def dropping(KD, name, rate=dr.RATE):
    """A fresh model with ``dropout_rate`` = rate and the synth weights of the dropout-free tiny config, in TRAINING mode, trainable."""
    from tests.test_unet_cpu import built
    _, _, sd = built(name)
    model = KD.config.make_model(KD.config.load_config(dr.dropping_config(name, rate)))
    model.load_state_dict(sd)
    return model.to(DEV).train()


def seeded(model, seed=SEED):
    """enable_dropout with a fresh device generator at ``seed``; returns the key the next loss call will draw."""
    model.enable_dropout(torch.Generator(device=DEV).manual_seed(seed))
    probe = torch.Generator(device=DEV).manual_seed(seed)
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=DEV, generator=probe).item())


def hip_loss(KD, model, name, weighting):
    x, noise, sigma, aug = tr.batch(name)
    kw = {} if aug is None else {"aug_cond": g(aug)}
    return KD.Denoiser(model, tr.SIGMA_DATA, weighting).loss(g(x), g(noise), g(sigma), **kw)


@functools.lru_cache(maxsize=None)
def restated(name, weighting, key):
    """(losses, {parameter name: gradient}, masks, conditioning) from autograd over the masked restatement under the Philox masks of ``key``:
    losses and gradients in fp64; conditioning = the worst max-abs relative error of the SAME restatement's fp32 gradients against them."""
    from tests.test_unet_cpu import built
    from tests.test_unet_drop_cpu import loss_and_grads
    _, _, sd = built(name)
    x, noise, sigma, aug = tr.batch(name)
    masks = dr.philox_masks(sd, key, dr.RATE, x.shape[0], tuple(x.shape[2:]))
    losses, grads = loss_and_grads(name, weighting, masks)
    keys = sorted(grads)
    leaves = tr.leaf_state(sd, set(keys), dtype=torch.float32)
    g32 = torch.autograd.grad(dr.losses(leaves, x, noise, sigma, aug, weighting, masks, dtype=torch.float32).mean(), [leaves[k] for k in keys])
    cond = max(((a.double() - grads[k]).abs().max() / grads[k].abs().max()).item() for k, a in zip(keys, g32))
    return losses, grads, masks, cond


@pytest.mark.parametrize("weighting", tr.WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_loss_and_parameter_gradients_match_fp64_under_dropout(KD, name, weighting):
    model = dropping(KD, name)
    key = seeded(model)
    want_losses, want, masks, cond = restated(name, weighting, key)
    # conditions on the case, from the numpy masks and the CPU restatement alone: a mask of all ones (or all zeros) cannot hide a wrong site,
    # and the reference's own fp32 arithmetic must not already spend the gate's headroom
    assert all(bool(m.any()) and not bool(m.all()) for m in masks), "a site without a dropped or without a kept element: choose another SEED"
    assert cond <= CASE_CONDITION, f"key {key}: the fp32 restatement is {cond:.2e} from fp64, an ill-conditioned case: choose another SEED"
    losses = hip_loss(KD, model, name, weighting)
    assert losses.shape == want_losses.shape and losses.requires_grad
    e_loss = ((losses.detach().cpu().double() - want_losses).abs() / want_losses.abs()).max().item()
    losses.mean().backward()
    grads = grads_of(model)
    assert sorted(grads) == sorted(want) and all(v is not None and v.shape == want[k].shape for k, v in grads.items())
    e_grad, k_grad = worst(grads, want)
    print(f"{name} {weighting} key {key}: losses {e_loss:.3e} (1e-5), worst gradient {e_grad:.3e} at {k_grad} (5e-4), {len(grads)} parameters, "
          f"{len(masks)} sites; the fp32 restatement {cond:.2e} ({CASE_CONDITION:.0e})")
    assert e_loss < 1e-5
    assert e_grad < 5e-4


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_seeds_eval_frozen_subsets_and_retained_graphs(KD, name):
    nat = KD._native
    model = dropping(KD, name)
    seeded(model)
    (losses, names) = profiled(nat, lambda: hip_loss(KD, model, name, "karras"))
    (_, back_names) = profiled(nat, lambda: losses.mean().backward())
    first = {k: v.clone() for k, v in grads_of(model).items()}
    for kernel in DROP_KERNELS:                                         # the training-mode loss runs every new kernel ...
        assert any(n.startswith(kernel) for n in names + back_names), (kernel, names + back_names)
    assert sum(n.startswith("chan_mask_f32") for n in names + back_names) == 1, "one table launch per loss call"
    # the next call draws another key: other masks, another loss
    second = hip_loss(KD, model, name, "karras")
    assert not torch.equal(second, losses)
    # the same seed: the same bits, losses and gradients
    model.zero_grad(set_to_none=True)
    seeded(model)
    again = hip_loss(KD, model, name, "karras")
    again.mean().backward()
    assert torch.equal(again, losses) and all(torch.equal(p.grad, first[k]) for k, p in model.named_parameters())
    # a retained graph: the second backward recomputes the tape with the same key -- exactly twice the first
    model.zero_grad(set_to_none=True)
    seeded(model)
    kept = hip_loss(KD, model, name, "karras").mean()
    kept.backward(retain_graph=True)
    kept.backward()
    assert all(torch.equal(p.grad, 2 * first[k]) for k, p in model.named_parameters()), "the second backward drew other masks"
    # a frozen subset under the same key: the same bits for the rest
    model.zero_grad(set_to_none=True)
    frozen = [k for k, _ in model.named_parameters() if ".main.2." in k or "mapping" in k or "proj_in" in k or k.endswith("qkv_proj.bias")]
    assert frozen and len(frozen) < len(first)
    for k, p in model.named_parameters():
        p.requires_grad_(k not in frozen)
    seeded(model)
    hip_loss(KD, model, name, "karras").mean().backward()
    for k, p in model.named_parameters():
        assert (p.grad is None) if k in frozen else torch.equal(p.grad, first[k]), f"{k}: other bits with a frozen subset"
    model.requires_grad_(True)
    # no grad mode: the same losses under the same key, no graph
    seeded(model)
    with torch.no_grad():
        plain = hip_loss(KD, model, name, "karras")
    assert not plain.requires_grad and torch.equal(plain, losses)
    # the default device generator serves when none is given: torch.manual_seed governs it
    model.enable_dropout()
    torch.manual_seed(5)
    a = hip_loss(KD, model, name, "karras").detach()
    torch.manual_seed(5)
    assert torch.equal(hip_loss(KD, model, name, "karras").detach(), a)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_eval_is_the_dropout_free_objective_and_names_no_new_kernel(KD, name):
    from tests.test_unet_train_gpu import trainable
    nat = KD._native
    model = dropping(KD, name)
    seeded(model)
    model.eval()
    clean = trainable(KD, name)                                         # dropout_rate 0, the same weights
    (losses, names) = profiled(nat, lambda: (lambda l: (l.mean().backward(), l)[1])(hip_loss(KD, model, name, "karras")))
    want = hip_loss(KD, clean, name, "karras")
    want.mean().backward()
    assert torch.equal(losses, want) and all(torch.equal(p.grad, q.grad) for p, q in zip(model.parameters(), clean.parameters()))
    assert not any(n.startswith(k) for n in names for k in DROP_KERNELS), names
    # a rate of 0 in training mode with dropout enabled: nothing applies, today's launches and bits
    clean.train().enable_dropout()
    clean.zero_grad(set_to_none=True)
    (l0, names0) = profiled(nat, lambda: (lambda l: (l.mean().backward(), l)[1])(hip_loss(KD, clean, name, "karras")))
    assert torch.equal(l0, want) and not any(n.startswith(k) for n in names0 for k in DROP_KERNELS)
    # forward_vjp (eval) names none of them either, and the sampling passes refuse training mode with a rate, enabled or not
    xi, si, aug = ur.inputs(name)
    kw = {} if aug is None else {"aug_cond": g(aug)}
    model.requires_grad_(False)
    u = g(rn(*xi.shape, seed=29))
    with torch.no_grad():
        (_, vjp_names) = profiled(nat, lambda: model.forward_vjp(g(xi), g(si), **kw)[1](u))
    assert vjp_names and not any(n.startswith(k) for n in vjp_names for k in DROP_KERNELS), vjp_names
    model.train()
    for call in (lambda: model(g(xi), g(si), **kw), lambda: model.forward_vjp(g(xi), g(si), **kw), lambda: model.forward_jvp(g(xi), g(si), g(xi), **kw)):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="dropout"):
            call()


def test_not_enabled_keeps_todays_refusal_on_the_device(KD):
    model = dropping(KD, "unet_b", rate=0.05)
    x, noise, sigma, _ = tr.batch("unet_b")
    with pytest.raises(NotImplementedError, match=r"dropout_rate=0\.05.*model\.eval\(\)"):
        KD.Denoiser(model, tr.SIGMA_DATA).loss(g(x), g(noise), g(sigma))
    assert KD.Denoiser(model.enable_dropout(), tr.SIGMA_DATA).loss(g(x), g(noise), g(sigma)).requires_grad

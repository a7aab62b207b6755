"""Dropout in the image_v1 U-Net's training loss, without a GPU: the restated masked loss (tests/unet_drop_ref.py) under fp64 autograd against the
REAL reference's recorded training-mode losses and gradient summaries under recorded masks (tests/golden/unet_drop.json), the ABI of the five
dropout entry points -- a fourth header (include/kdiff_unet_drop.h) with a binding table of its own (``_native.DROP_SIGNATURES``), so that the
three pinned tables stay as they are -- the site list, the numpy statement of the mask contract that the GPU tests import, ``enable_dropout``'s
argument checks and the refusals that need no device."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import unet_drop_ref as dr
from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.test_unet_cpu import built

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_unet_drop.h")
ENTRY_POINTS = {"kd_chan_mask_f32": 9, "kd_conv2d_x3_drop": 17, "kd_chan_scale_f32": 10, "kd_attn_global_drop_f32": 10,
                "kd_attn_global_drop_vjp_f32": 13}
# The gap between the restatement and the reference, both in fp64 under the same masks, x 100.  Measured here: 0 -- the golden's stand-ins and the
# restatement spell the same torch expressions, so on one torch build they agree bit for bit -- and 100 x 0 gates nothing but that build.  The gate
# is therefore the one of the dropout-free restatement (tests/test_unet_train_cpu.py: 100 x its measured 6.5e-16, where torch's own SDPA and the
# spelt-out softmax differ in the order of their roundings): what another order of the same fp64 operations can move.  Far below the fp32
# reference's own gradient error against fp64, 1e-6
GATE = 6.5e-14


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(REPO, "tests", "golden", "unet_drop.json")))


def loss_and_grads(name, weighting, masks, rate=dr.RATE):
    """(losses, {parameter name: gradient}) of ``losses.mean()`` in fp64 from autograd over the masked restatement."""
    _, model, sd = built(name)
    names = {k for k, _ in model.named_parameters()}
    leaves = tr.leaf_state(sd, names)
    x, noise, sigma, aug = tr.batch(name)
    losses = dr.losses(leaves, x, noise, sigma, aug, weighting, masks, rate)
    keys = sorted(names)
    grads = torch.autograd.grad(losses.mean(), [leaves[k] for k in keys])
    return losses.detach(), dict(zip(keys, grads))


@pytest.mark.parametrize("weighting", tr.WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_restatement_reproduces_the_golden(name, weighting):
    """Losses, gradient norms and probe products of the masked restatement against the real reference's in training mode, fp64 both, under the
    recorded masks.  Measured (relative; the probe product relative to norm * |probe|): losses, norms and probe products all 0 over both
    configs and the three weightings (the same torch expressions in the same order: see GATE for why the gate is 6.5e-14 and not 100 x 0)."""
    gold = golden()[name]
    assert gold["rate"] == dr.RATE
    _, _, sd = built(name)
    sites = dr.site_list(sd)
    masks = [dr.unpack(m) for m in gold["masks"]]
    assert [(m["kind"], m["prefix"]) for m in gold["masks"]] == [(kind, prefix) for _, kind, prefix in sites]
    assert all(m.dim() == (4 if kind == "attn" else 2) and bool(m.any()) and not bool(m.all()) for m, (_, kind, _) in zip(masks, sites))
    losses, grads = loss_and_grads(name, weighting, masks)
    gold = gold[weighting]
    assert GATE < 1e-6
    assert sorted(grads) == sorted(gold["grads"]) and len(grads) == {"unet_a": 84, "unet_b": 72}[name]
    want = torch.tensor(gold["losses"], dtype=torch.float64)
    e_loss = ((losses - want).abs() / want.abs()).max().item()
    e_norm = e_probe = 0.0
    for k, g in grads.items():
        norm, dot = tr.summary(g)
        w_norm, w_dot = gold["grads"][k]
        assert w_norm > 0
        e_norm = max(e_norm, abs(norm - w_norm) / w_norm)
        e_probe = max(e_probe, abs(dot - w_dot) / (w_norm * tr.probe(g.numel()).norm().item()))
    print(f"{name} {weighting}: losses {e_loss:.3e}, norms {e_norm:.3e}, probe products {e_probe:.3e} (gate {GATE:.1e})")
    assert e_loss < GATE and e_norm < GATE and e_probe < GATE


def test_the_masks_matter_and_all_ones_is_the_plain_restatement():
    """The masked restatement with every element kept at rate 0 is tests/unet_ref.py's forward; the recorded masks move the loss."""
    name = "unet_b"
    _, _, sd = built(name)
    x, noise, sigma, aug = tr.batch(name)
    sd64 = tr.leaf_state(sd, set())
    ones = [torch.ones_like(dr.unpack(m)) for m in golden()[name]["masks"]]
    plain = tr.losses(sd64, x, noise, sigma, aug, "karras")
    assert torch.allclose(dr.losses(sd64, x, noise, sigma, aug, "karras", ones, rate=0.0), plain, rtol=1e-13, atol=0)
    dropped = dr.losses(sd64, x, noise, sigma, aug, "karras", [dr.unpack(m) for m in golden()[name]["masks"]])
    assert ((dropped - plain).abs() / plain).min().item() > 1e-3


def header_parameters():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kd_\w+)\s*\((.*?)\)\s*;", src, flags=re.S):
        out[name] = [tuple(re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a).groups()) for a in args.split(",")]
    return out


def _kind(ctype):
    t = ctype.replace("const", "").strip()
    if "*" in t:
        return C.c_void_p
    return {"float": C.c_float, "int": C.c_int, "unsigned": C.c_uint, "unsigned long long": C.c_ulonglong, "long long": C.c_longlong}[t]


def test_the_library_exports_and_binds_what_the_header_declares(KD):
    nat = KD._native
    params = header_parameters()
    assert sorted(params) == sorted(ENTRY_POINTS) == sorted(nat.DROP_SIGNATURES) == sorted(nat.DROP_RESTYPES)
    parsed = KD._abi.parse(open(HEADER).read())
    assert not parsed.structs and not parsed.constants
    lib = nat.lib()
    for name, n_args in ENTRY_POINTS.items():
        kinds = [_kind(t) for t, _ in params[name]]
        assert len(kinds) == n_args and kinds == nat.DROP_SIGNATURES[name] == parsed.signatures[name], name
        assert kinds[-1] is C.c_void_p and params[name][-1][1] == "stream"
        fn = getattr(lib, name)                                        # exported ...
        assert list(fn.argtypes) == kinds and fn.restype is C.c_int    # ... and bound with the parsed types
    # the other three tables stay what they were: none of the new names, and no run-list op for them
    others = set(nat.SIGNATURES) | set(nat.GRAD_SIGNATURES) | set(nat.TRAIN_SIGNATURES) | set(nat.RUN_LIST_OPS)
    assert not set(ENTRY_POINTS) & others
    for header in ("kdiff_hip.h", "kdiff_unet_grad.h", "kdiff_unet_train.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in ENTRY_POINTS)
    # the new kernels' file reads no library option and calls no atomic; the two shared files gained neither
    csrc = os.path.join(REPO, "k-diffusion_amd", "csrc")
    text = open(os.path.join(csrc, "unet_drop_f32.hip")).read()
    assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)|\batomic\w*\s*\(", text)
    for src in ("conv_x3.hip", "vjp_f32.hip"):
        assert not re.findall(r"\bopt(?:_or)?\(|\batomic\w*\s*\(", open(os.path.join(csrc, src)).read()), src
    assert "unet_drop_f32.o" in open(os.path.join(csrc, "Makefile")).read()
    # wrappers live in unet_ops, not in ops (tests/test_guard_cpu.py wants a case in tests/test_bounds_gpu.py for everything there)
    for wrapper in ("chan_mask", "chan_layout", "chan_scale", "attn_global_drop", "attn_global_drop_vjp", "drop_factors"):
        assert callable(getattr(KD.unet_ops, wrapper)) and wrapper not in vars(KD.ops)


def _drop_model(KD, name, rate=0.05):
    return KD.config.make_model(KD.config.load_config(dr.dropping_config(name, rate)))


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_dropout_sites_order_ids_and_disjointness(KD, name):
    model = _drop_model(KD, name)
    inner = getattr(model, "inner_model", model)
    import sys
    v1 = sys.modules[type(inner).__module__]                           # the copy of the module the model's classes come from (nothing new is imported)
    sites = v1.dropout_sites(inner)
    layers = v1.forward_layers(inner)
    mods = dict(inner.named_modules())
    # order and ids: the independent walk of the state dict's names (tests/unet_drop_ref.py) gives the same list
    want = dr.site_list(inner.state_dict())
    assert [(s, kind) for s, _, kind, _ in sites] == [(s, kind) for s, kind, _ in want]
    assert [layer for _, layer, _, _ in sites] == [mods[prefix[:-1]] for _, _, prefix in want]
    at = 0
    for L, layer in enumerate(layers):
        base = 1 << 62 | 1 << 33 | 2 * L
        if hasattr(layer, "qkv_proj"):
            assert sites[at][0] == base and sites[at][1] is layer and sites[at][2:] == ("attn", layer.c_in)
            at += 1
        else:
            assert sites[at][0] == base and sites[at][2:] == ("conv1", layer.c_mid)
            assert sites[at + 1][0] == base + 1 and sites[at + 1][1] is layer and sites[at + 1][2:] == ("conv2", layer.c_out)
            at += 2
    assert at == len(sites) == len(golden()[name]["masks"])
    ids = [s for s, *_ in sites]
    assert len(set(ids)) == len(ids)
    assert all(s >> 62 == 1 and s >> 33 & 1 for s in ids), "bit 62 set, bit 63 clear, bit 33 set"
    # disjoint from every id the transformer's dropout_sites can give: 2^62 | 2 i, 2^62 | (2 i + 1) (a layer position: far below 2^31)
    # and 2^62 | 2^32 | k (a mapping block: far below 2^32) all have bit 33 clear
    v2 = KD.models.image_transformer_v2
    assert v2.DROPOUT_SITE == 1 << 62
    for i in (0, 1, 2 ** 31 - 1):
        for other in (v2.DROPOUT_SITE | 2 * i, v2.DROPOUT_SITE | (2 * i + 1), v2.DROPOUT_SITE | 1 << 32 | i, v2.DROPOUT_SITE | 1 << 32 | (2 * i + 1)):
            assert not other >> 33 & 1 and other not in ids


def test_enable_dropout_argument_checks(KD):
    model = _drop_model(KD, "unet_b")
    before = sorted(model.state_dict())
    assert model.enable_dropout() is model and model._dropout_on and model._dropout_gen is None
    gen = torch.Generator().manual_seed(1)
    assert model.enable_dropout(gen) is model and model._dropout_gen is gen
    assert sorted(model.state_dict()) == before, "the setting is not part of the state_dict"
    with pytest.raises(TypeError, match="torch.Generator or None"):
        model.enable_dropout(generator=7)
    for bad in (1.0, -0.1, 1.5):
        broken = _drop_model(KD, "unet_b")
        broken.dropout_rate = bad
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            broken.enable_dropout()
        assert not broken._dropout_on
    # the wrapper delegates and returns itself
    wrapped = _drop_model(KD, "unet_a")
    assert wrapped.enable_dropout(gen) is wrapped and wrapped.inner_model._dropout_on and wrapped.inner_model._dropout_gen is gen
    with pytest.raises(TypeError, match="torch.Generator or None"):
        wrapped.enable_dropout("seed")
    # a rate of 0 may be enabled: nothing applies
    plain = KD.config.make_model(built("unet_b")[0]).enable_dropout()
    assert plain._dropout_on and not plain._dropout_applies()


def test_refusals_without_a_device(KD):
    x, noise, sigma, _ = tr.batch("unet_b")
    model = _drop_model(KD, "unet_b")
    assert model.training and model.dropout_rate == 0.05
    # not enabled: today's refusal, with today's message
    with pytest.raises(NotImplementedError, match=r"dropout_rate=0\.05.*model\.eval\(\)"):
        model.loss_forward(x, sigma)
    model.enable_dropout()
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # enabled: the loss goes through to the operand checks
        model.loss_forward(x, sigma)
    model.requires_grad_(False)
    for call in (lambda: model(x, sigma), lambda: model.forward_jvp(x, sigma, x), lambda: model.forward_vjp(x, sigma)):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="dropout"):     # the sampling passes have none, enabled or not
            call()
    model.eval()
    for call in (lambda: model(x, sigma), lambda: model.forward_vjp(x, sigma), lambda: model.loss_forward(x, sigma)):
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):    # eval(): the dropout-free passes go through
            call()
    wrapped = _drop_model(KD, "unet_a")
    xa, _, sa, aug = tr.batch("unet_a")
    with pytest.raises(NotImplementedError, match=r"dropout_rate=0\.05.*model\.eval\(\)"):
        wrapped.loss_forward(xa, sa, aug_cond=aug)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wrapped.enable_dropout().loss_forward(xa, sa, aug_cond=aug)
    # train.py keeps refusing the family
    src = open(os.path.join(REPO, "train.py")).read()
    assert re.search(r"model_config\['type'\] == 'image_v1':\s+raise NotImplementedError\('[^']*Denoiser\.loss", src)


def test_the_numpy_mask_contract():
    """``unet_drop_ref``'s statement of include/kdiff_unet_drop.h, which the GPU tests hold the kernels to: the generator's known answer, the
    element orders, the threshold and the scale."""
    from oracle.brownian import philox4x32_10
    # Random123's known answer for philox4x32-10 with counter and key all ones
    words = philox4x32_10(0xFFFFFFFFFFFFFFFF, np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF), 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(np.asarray(w).reshape(-1)[0]) for w in words] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    key, site, p = -5, dr.SITE | 6, 0.25
    flat = dr.keep_flags(key, site, p, 3 * 128)
    assert flat.dtype == bool and np.array_equal(dr.chan_keep(key, site, p, 3, 128), flat.reshape(3, 128))
    assert np.array_equal(dr.keep_flags(key, site, p, 50), flat[:50]) and not np.array_equal(dr.keep_flags(key, site + 1, p, 384), flat)
    assert not np.array_equal(dr.keep_flags(key + 1, site, p, 384), flat)
    assert np.array_equal(dr.keep_flags(key + 2 ** 64, site, p, 384), flat), "the key is taken as its 64 bits"
    # word e & 3 of the block at counter e >> 2, threshold floor(p 2^32): spelt out for single elements
    for e in (0, 5, 383):
        w = philox4x32_10(key & (2 ** 64 - 1), np.uint64(e >> 2), np.uint64(0), site & 0xFFFFFFFF, site >> 32)[e & 3]
        assert bool(flat[e]) == (int(np.asarray(w).reshape(-1)[0]) >= int(0.25 * 2 ** 32))
    # an attention row starts on a counter boundary: T = 49 pads every row to 52 elements
    B, nh, T = 2, 2, 49
    m = dr.attn_keep(key, site, p, B, nh, T)
    padded = dr.keep_flags(key, site, p, B * nh * T * 52).reshape(B, nh, T, 52)
    assert m.shape == (B, nh, T, T) and np.array_equal(m, padded[..., :T])
    assert np.array_equal(dr.attn_keep(key, site, p, B, nh, 64), dr.keep_flags(key, site, p, B * nh * 64 * 64).reshape(B, nh, 64, 64))
    assert dr.scale_of(0.25) == np.float32(4.0 / 3.0) and dr.scale_of(0.05) == np.float32(1.0 / 0.95) and dr.scale_of(0.5) == np.float32(2.0)
    # the dropped fraction at 2^16 elements, within 5 binomial standard deviations
    for rate in (0.05, 0.5):
        frac = 1.0 - dr.keep_flags(123, site, rate, 2 ** 16).mean()
        assert abs(frac - rate) < 5 * (rate * (1 - rate) / 2 ** 16) ** 0.5
    # packing is lossless
    t = torch.from_numpy(m)
    assert torch.equal(dr.unpack(dr.pack(t)), t)
    # the masks of a whole model: one per site, the shapes the restatement takes
    _, _, sd = built("unet_a")
    masks = dr.philox_masks(sd, 77, dr.RATE, 3, (12, 20))
    assert [tuple(x.shape) for x in masks] == [tuple(r["shape"]) for r in golden()["unet_a"]["masks"]]

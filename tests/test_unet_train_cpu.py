"""Training the image_v1 U-Net, without a GPU: the restated loss (tests/unet_train_ref.py over tests/unet_ref.py) under fp64 autograd against the
REAL reference's recorded losses and gradient summaries (tests/golden/unet_train.json), the ABI of the four parameter-gradient entry points --
a third header (include/kdiff_unet_train.h) with a binding table of its own (``_native.TRAIN_SIGNATURES``), so that the two pinned tables stay
as they are -- the chunking rule of the convolution's weight gradient, and the refusals of ``loss_forward`` that need no device."""
import ctypes as C
import functools
import json
import os
import re

import pytest
import torch

from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.test_unet_cpu import built

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_unet_train.h")
ENTRY_POINTS = {"kd_conv2d_wgrad_x3": 17, "kd_adagn_wb_grad_f32": 15, "kd_gelu_vjp_f32": 5, "kd_bias_grad_f32": 10}
# The gap between the restatement and the reference, both in fp64 (measured: see test_restatement_reproduces_the_golden), x 100 -- and in any case
# below the fp32 reference's own gradient error against fp64, 1e-6
GATE = 6.5e-14


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(REPO, "tests", "golden", "unet_train.json")))


@functools.lru_cache(maxsize=None)
def restated(name, weighting):
    """(losses, {parameter name: gradient}) of ``losses.mean()`` in fp64 from autograd over the restatement: computed once, shared."""
    cfg, model, sd = built(name)
    names = {k for k, _ in model.named_parameters()}
    leaves = tr.leaf_state(sd, names)
    x, noise, sigma, aug = tr.batch(name)
    losses = tr.losses(leaves, x, noise, sigma, aug, weighting)
    keys = sorted(names)
    grads = torch.autograd.grad(losses.mean(), [leaves[k] for k in keys])
    return losses.detach(), dict(zip(keys, grads))


@pytest.mark.parametrize("weighting", tr.WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_restatement_reproduces_the_golden(name, weighting):
    """Losses, gradient norms and probe products of the restatement against the real reference's, fp64 both.  Measured (relative; the probe
    product relative to norm * |probe|): losses <= 4.3e-16, norms <= 6.5e-16, probe products <= 2.9e-16 over both configs and the three
    weightings; the gate is 100 x the largest, 6.5e-14, far below the 1e-6 of the fp32 reference's own gradient error."""
    gold = golden()[name][weighting]
    losses, grads = restated(name, weighting)
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


def header_parameters():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kd_\w+)\s*\((.*?)\)\s*;", src, flags=re.S):
        out[name] = [tuple(re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a).groups()) for a in args.split(",")]
    return out


def test_the_library_exports_and_binds_what_the_header_declares(KD):
    nat = KD._native
    params = header_parameters()
    assert sorted(params) == sorted(ENTRY_POINTS) == sorted(nat.TRAIN_SIGNATURES) == sorted(nat.TRAIN_RESTYPES)
    parsed = KD._abi.parse(open(HEADER).read())
    assert not parsed.structs and not parsed.constants
    lib = nat.lib()
    for name, n_args in ENTRY_POINTS.items():
        kinds = [C.c_void_p if "*" in t else (C.c_float if t.strip().startswith("float") else C.c_int) for t, _ in params[name]]
        assert len(kinds) == n_args and kinds == nat.TRAIN_SIGNATURES[name] == parsed.signatures[name], name
        assert kinds[-1] is C.c_void_p and params[name][-1][1] == "stream"
        fn = getattr(lib, name)                                        # exported ...
        assert list(fn.argtypes) == kinds and fn.restype is C.c_int    # ... and bound with the parsed types
    # the other two tables stay what they were: none of the new names, and no run-list op for them
    others = set(nat.SIGNATURES) | set(nat.GRAD_SIGNATURES) | set(nat.RUN_LIST_OPS)
    assert not set(ENTRY_POINTS) & others
    for header in ("kdiff_hip.h", "kdiff_unet_grad.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in ENTRY_POINTS)
    # the new kernels read no library option and call no atomic
    for src in ("conv_wgrad_x3.hip", "unet_train_f32.hip"):
        text = open(os.path.join(REPO, "k-diffusion_amd", "csrc", src)).read()
        assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)|\batomic\w*\s*\(", text)
    # wrappers live in unet_ops, not in ops (tests/test_guard_cpu.py wants a case in tests/test_bounds_gpu.py for everything there)
    for wrapper in ("conv2d_wgrad", "conv_wgrad_chunks", "adagn_wb_grad", "gelu_vjp", "bias_grad"):
        assert callable(getattr(KD.unet_ops, wrapper)) and wrapper not in vars(KD.ops)


def test_the_chunking_is_a_function_of_the_shape(KD):
    chunks = KD.unet_ops.conv_wgrad_chunks
    for B, H, W, ci, co in ((2, 12, 20, 64, 128), (1, 2, 2, 64, 64), (64, 32, 32, 128, 128), (3, 7, 7, 128, 64), (5, 24, 8, 64, 64), (64, 8, 8, 256, 256)):
        patches = B * -(-H // 8) * -(-W // 8)
        per, n = chunks(B, H, W, ci, co)
        assert (per, n) == chunks(B, H, W, ci, co)
        assert per >= 1 and n >= 1 and (n - 1) * per < patches <= n * per, (B, H, W, ci, co, per, n)
    assert chunks(1, 2, 2, 64, 64) == (1, 1)
    per, n = chunks(5, 56, 8, 256, 256)                                 # the GPU test's multi-chunk shape: >= 3 chunks, the last one ragged
    assert n >= 3 and 35 % per


def test_loss_forward_refusals_without_a_device(KD):
    cfg, model, _ = built("unet_b")
    x, noise, sigma, _ = tr.batch("unet_b")
    trainable = KD.config.make_model(cfg)                              # training mode, parameters that require grad, dropout_rate 0
    assert trainable.training and trainable.dropout_rate == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # not "sampling only": loss_forward takes trainable parameters
        trainable.loss_forward(x, sigma)
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):     # the forward's refusal is unchanged
        trainable(x, sigma)
    with pytest.raises(NotImplementedError, match="input gets no gradient"):
        trainable.loss_forward(x.clone().requires_grad_(True), sigma)
    with pytest.raises(NotImplementedError, match="sigma gets no gradient"):
        trainable.loss_forward(x, sigma.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="unet_cond"):
        trainable.loss_forward(x, sigma, unet_cond=x)
    raw = json.loads(json.dumps(ur.CONFIGS["unet_b"]))
    raw["model"]["dropout_rate"] = 0.05
    dropping = KD.config.make_model(KD.config.load_config(raw))
    with pytest.raises(NotImplementedError, match=r"dropout_rate=0\.05.*model\.eval\(\)"):
        dropping.loss_forward(x, sigma)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # eval(): the dropout-free objective goes through
        dropping.eval().loss_forward(x, sigma)
    # the wrapper has the rule, with the conditioning rule of forward_preconditioned
    wrapped = KD.config.make_model(built("unet_a")[0])
    xa, _, sa, aug = tr.batch("unet_a")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wrapped.loss_forward(xa, sa, aug_cond=aug)
    with pytest.raises(NotImplementedError, match="mapping_cond gets no gradient"):
        wrapped.loss_forward(xa, sa, aug_cond=aug.clone().requires_grad_(True))
    src = open(os.path.join(REPO, "train.py")).read()
    assert re.search(r"model_config\['type'\] == 'image_v1':\s+raise NotImplementedError\('[^']*Denoiser\.loss", src)

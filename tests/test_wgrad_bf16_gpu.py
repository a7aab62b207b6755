"""bf16 weight-gradient arithmetic on the MI355X (``ops.wgrad(bf16=True)``, ``set_wgrad_arithmetic("bf16")``, ``train.py --mixed-precision
bf16``): the kernel against the fp64 product of the bf16-rounded operands, the model's gradients against fp64 autograd through the oracle
within the reference's own bf16 error, the untouched bits of everything else, and train.py end to end.

Kernel bound: truth is Gb^T Ab in fp64, Gb / Ab the operands after their whole prologue rounded to bf16 on the CPU; the yardstick is the same
product by torch in fp32 on the CPU; the kernel may miss the truth by 4 x the yardstick's miss (the 4 x convention of
tests/test_training_gpu.py).  The inputs are random normals (not bf16-representable), so a split3 result lies ~2^-9 relative away: orders
of magnitude outside the bound.

The GEGLU case takes the fp32 operand from the device (``_device_geglu``: the last-bit difference between the device's erff and the
CPU's erf would otherwise flip bf16 roundings).  The dropout form masks A's plain rows, so the cases that gather A (the kernels refuse a mask there) run in the plain form only."""
import functools
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.golden import cases
from tests.helpers import relerr
from tests.test_param_grad_gpu import _hip_loss, _inputs, _model, _oracle_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = cases.REPO
P_DROP = 0.25
SITE = (1 << 62) | 77


def g(t):
    return t.to(DEV, torch.float32).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _gelu_rows(u):
    d = u.shape[-1] // 2
    return u[..., :d] * torch.nn.functional.gelu(u[..., d:])


def _merge_rows(fine, gh, gw):
    B, _, _, C = fine.shape
    return fine.view(B, gh, 2, gw, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, 4 * C)


def _patch_rows(img, gh, gw, ph, pw):
    B, C = img.shape[:2]
    return img.permute(0, 2, 3, 1).reshape(B, gh, ph, gw, pw, C).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, ph * pw * C)


def _device_geglu(U):
    """value * gelu(gate) in fp32 as the device evaluates it, read back through the exact-fp32 weight gradient of an identity G (every
    sum is one operand element times 1.0 plus zeros: exact).  The device's erff and the CPU's erf differ in the last fp32 bit on some
    elements, and such an element next to a bf16 rounding boundary rounds the other way: one flip moves an entry of the product by 2^-9 of
    that element, 10 .. 100 x the fp32 yardstick, although no arithmetic of the GEMM is off.  So the operand 'after its prologue' is the
    device's fp32 value (from the fp32-FMA kernel, not the one under test), held to the CPU's GEGLU within fp32 rounding here, and rounded
    to bf16 on the CPU like every other operand."""
    KD = importlib.import_module("k_diffusion_amd")
    M = U.shape[0]
    dev = KD.ops.wgrad(torch.eye(M, device=DEV), g(U), geglu=True, precision=KD.ops.nat.PREC_EXACT).cpu()
    cpu = _gelu_rows(U)
    d = U.shape[-1] // 2
    scale = cpu.abs() + (U[:, :d] * U[:, d:]).abs()          # 1 + erf(gate) cancels for negative gates: its error is absolute
    assert ((dev - cpu).abs() <= 4e-7 * scale).all(), ((dev - cpu).abs() / scale).max()
    return dev


def _case(name, nat):
    """(G, A as passed, ops.wgrad keywords, the fp32 operands after their prologue [M, N] / [M, K], whether A's rows are plain)."""
    gen = _gen(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    if name.startswith("plain"):                    # plain_M_N_K
        M, N, K = map(int, name.split("_")[1:])
        G, A = rn(M, N), rn(M, K)
        return G, A, {}, G, A, True
    if name == "merge_g":
        fine, A = rn(2, 4, 4, 8), rn(8, 40)
        return fine, A, dict(gather=("g", nat.WG_MERGE2x2), gather_geom=(2, 2, 2, 2, 8)), _merge_rows(fine, 2, 2), A, True
    if name == "merge_a":
        G, fine = rn(8, 72), rn(2, 4, 4, 8)
        return G, fine, dict(gather=("a", nat.WG_MERGE2x2), gather_geom=(2, 2, 2, 2, 8)), G, _merge_rows(fine, 2, 2), False
    if name == "patch_g":
        img, A = rn(2, 3, 4, 4), rn(8, 40)
        return img, A, dict(gather=("g", nat.WG_PATCH_NCHW), gather_geom=(2, 2, 2, 2, 3)), _patch_rows(img, 2, 2, 2, 2), A, True
    if name == "patch_a":
        G, img = rn(8, 72), rn(2, 3, 4, 4)
        return G, img, dict(gather=("a", nat.WG_PATCH_NCHW), gather_geom=(2, 2, 2, 2, 3)), G, _patch_rows(img, 2, 2, 2, 2), False
    if name == "geglu":
        G, U = rn(200, 72), rn(200, 80) * 2
        return G, U, dict(geglu=True), G, _device_geglu(U), True
    if name == "scales":
        M, N, K = 200, 72, 40
        G, A = rn(M, N), rn(M, K)
        rr, cs = torch.rand(M, generator=gen) + 0.5, torch.rand(2, K, generator=gen) + 0.5
        return (G, A, dict(row_scale=g(rr), col_scale=g(cs), rows_per_sample=M // 2), G,
                (A * rr[:, None]) * cs.repeat_interleave(M // 2, 0), True)
    raise KeyError(name)


def _check(out, Gop, Aop, name, base=None, alpha=None):
    """max|hip - fp64| <= 4 max|torch fp32 - fp64| on the product of the bf16-rounded operands."""
    Gb, Ab = Gop.bfloat16(), Aop.bfloat16()
    truth = Gb.double().T @ Ab.double()
    yard = Gb.float().T @ Ab.float()
    if base is not None:
        truth = base.double() + float(alpha) * truth
        yard = base + alpha * yard
    err, err_yard = (out.cpu().double() - truth).abs().max().item(), (yard.double() - truth).abs().max().item()
    print(f"{name}: |hip - fp64| {err:.3e}  |torch fp32 - fp64| {err_yard:.3e}  ratio {err / err_yard:.2f}  (|truth| max {truth.abs().max():.3e})")
    assert err <= 4 * err_yard, (name, err, err_yard)


def _mask(KD, shape, key):
    """The site's mask values (scale or 0) as ``ops.dropout`` applies them."""
    return KD.ops.dropout(torch.ones(shape, device=DEV), key, SITE, P_DROP).cpu()


# the two element paths (columns a multiple of 4 or not), several chunks with a last one that is not full (M = 200), a ragged last
# 32-row step (M = 70), more than one 128-wide tile in both directions with ragged edges
KERNEL_CASES = ["plain_200_72_40", "plain_70_72_40", "plain_200_71_39", "plain_70_136_260", "merge_g", "merge_a", "patch_g", "patch_a",
                "geglu", "scales"]


@pytest.mark.parametrize("form", ["plain", "drop"])
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_against_rounded_operand_product(KD, name, form):
    G, A, kw, Gop, Aop, a_plain = _case(name, KD.ops.nat)
    if form == "drop":
        if not a_plain:
            with pytest.raises(ValueError, match="plain A rows"):
                KD.ops.wgrad(g(G), g(A), bf16=True, dropout=(torch.tensor([5], device=DEV), SITE, P_DROP), **kw)
            return
        key = torch.tensor([1234567 + len(name)], dtype=torch.int64, device=DEV)
        mask = _mask(KD, Aop.shape, key)
        assert 0 < (mask == 0).float().mean() < 0.5
        # the mask multiplies the plain (GEGLU'd) operand before the row and column scales
        if name == "scales":
            rr, cs = kw["row_scale"].cpu(), kw["col_scale"].cpu()
            Aop = ((A * mask) * rr[:, None]) * cs.repeat_interleave(A.shape[0] // 2, 0)
        else:
            Aop = Aop * mask
        kw = dict(kw, dropout=(key, SITE, P_DROP))
    out = KD.ops.wgrad(g(G), g(A), bf16=True, **kw)
    _check(out, Gop, Aop, f"{name}/{form}")
    assert torch.equal(out, KD.ops.wgrad(g(G), g(A), bf16=True, **kw)), "repeat call"
    if form == "drop":                              # p = 0: the plain call's bits
        plain = {k: v for k, v in kw.items() if k != "dropout"}
        assert torch.equal(KD.ops.wgrad(g(G), g(A), bf16=True, **plain),
                           KD.ops.wgrad(g(G), g(A), bf16=True, **dict(plain, dropout=(kw["dropout"][0], SITE, 0.0))))


def test_alpha_and_accumulate(KD):
    G, A, _, Gop, Aop, _ = _case("plain_200_72_40", KD.ops.nat)
    base = torch.randn(72, 40, generator=_gen(3))
    alpha = torch.tensor([0.75])
    acc = g(base)
    KD.ops.wgrad(g(G), g(A), out=acc, accumulate=True, alpha=g(alpha), bf16=True)
    _check(acc, Gop, Aop, "alpha/accumulate", base=base, alpha=alpha)
    acc2 = g(base)
    KD.ops.wgrad(g(G), g(A), out=acc2, accumulate=True, alpha=g(alpha), bf16=True)
    assert torch.equal(acc, acc2)


@pytest.mark.parametrize("mode", ["split3", "exact"])
def test_bf16_false_keeps_the_bits(KD, mode):
    nat = KD.ops.nat
    prec = nat.PREC_SPLIT3 if mode == "split3" else nat.PREC_EXACT
    for name in ("plain_200_72_40", "geglu", "merge_a"):
        G, A, kw, *_ = _case(name, nat)
        a = KD.ops.wgrad(g(G), g(A), precision=prec, **kw)
        assert torch.equal(a, KD.ops.wgrad(g(G), g(A), precision=prec, bf16=False, **kw)), name
        assert not torch.equal(a, KD.ops.wgrad(g(G), g(A), precision=prec, bf16=True, **kw)), name
    G, A, kw, *_ = _case("plain_200_72_40", nat)
    assert torch.equal(KD.ops.wgrad(g(G), g(A), precision=nat.PREC_BF16), KD.ops.wgrad(g(G), g(A), precision=nat.PREC_SPLIT3))


# ---------------------------------------------------------------------------------------------------------- the model

@functools.lru_cache(maxsize=None)
def _reference(KD, name):
    """fp64 autograd through the oracle, once per config, as tests/test_param_grad_gpu.py obtains it; read-only."""
    cfg, model, sd = _model(KD, name)
    x, noise, sigma, kw = _inputs(cfg, 2)
    return _oracle_loss(cfg, model, sd, x, noise, sigma, kw)


def _clone(grads):
    return {n: t.clone() for n, t in grads.items()}


@pytest.mark.parametrize("name", ["tiny_global", "tiny_sw", "tiny_na"])
def test_model_gradients_within_the_references_bf16_error(KD, monkeypatch, name):
    """Per parameter: max|g - g_fp64| / max|g_fp64| <= max(err_ref[name], 3e-4), err_ref the reference's own bf16-autocast error
    (tests/golden/wgrad_bf16.json), 3e-4 the split3 bound for tensors that pass no weight-gradient GEMM."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    err_ref = json.load(open(os.path.join(cases.GOLDEN_DIR, "wgrad_bf16.json")))[name]
    cfg, model, _ = _model(KD, name)
    x, noise, sigma, kw = _inputs(cfg, 2)
    _, ref_g = _reference(KD, name)
    loss0, g0 = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    g0 = _clone(g0)
    assert model.set_wgrad_arithmetic("bf16") is model
    loss1, g1 = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    g1 = _clone(g1)
    assert torch.equal(loss0, loss1)                # the primal stays fp32-grade
    worst, misses, moved = ("", 0.0), {}, 0
    for n, ref in ref_g.items():
        e = relerr(g1[n], ref)
        bound = max(err_ref[n], 3e-4)
        moved += not torch.equal(g0[n], g1[n])
        if e / bound > worst[1]:
            worst = (n, e / bound)
        if not e <= bound:
            misses[n] = (e, err_ref[n])
    print(f"{name}: worst error / bound {worst[1]:.3f} ({worst[0]}); {moved} of {len(ref_g)} gradients moved")
    assert moved > len(ref_g) // 3                  # the projections' gradients did take the new arithmetic
    assert not misses, misses
    # the input gradient's bits do not move either
    vjp = importlib.import_module(KD.__name__ + ".models.vjp")
    gout = torch.randn(x.shape, generator=_gen(3)).to(DEV)
    dkw = {k: v.to(DEV) for k, v in kw.items()}
    gx1, _ = vjp.backward(model, g(x), g(sigma), gout, params=list(model.parameters()), **dkw)
    model.set_wgrad_arithmetic(None)
    gx0, _ = vjp.backward(model, g(x), g(sigma), gout, params=list(model.parameters()), **dkw)
    assert torch.equal(gx0, gx1)
    # switched off again: a fresh model's bits
    _, g2 = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    _, fresh, _ = _model(KD, name)
    _, g3 = _hip_loss(KD, fresh, cfg, x, noise, sigma, kw)
    for n in g0:
        assert torch.equal(g2[n], g0[n]) and torch.equal(g2[n], g3[n]), n


def test_bf16_request_is_honoured_under_exact(KD, monkeypatch):
    monkeypatch.setenv("KDIFF_GEMM", "exact")
    cfg, model, _ = _model(KD, "tiny_global")
    x, noise, sigma, kw = _inputs(cfg, 2)
    _, g0 = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    g0 = _clone(g0)
    model.set_wgrad_arithmetic("bf16")
    _, g1 = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    n = "levels.0.0.ff.up_proj.weight" if "levels.0.0.ff.up_proj.weight" in g0 else next(k for k in g0 if k.endswith("up_proj.weight"))
    e = relerr(g1[n], g0[n])
    assert 1e-5 < e < 2e-2, e                       # bf16 operands: far from fp32 FMAs, close to the gradient


# ---------------------------------------------------------------------------------------------------------- train.py

def _run_train(cwd, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


def test_train_py_mixed_precision_bf16(KD, tmp_path):
    from PIL import Image
    data_dir = tmp_path / "images"
    data_dir.mkdir()
    gen = _gen(8)
    for i in range(4):
        arr = (torch.rand(16, 16, 3, generator=gen) * 255).to(torch.uint8).numpy()
        Image.fromarray(arr, mode="RGB").save(data_dir / f"img_{i:02}.png")
    config = cases.raw_config("tiny_global")
    config["model"].update({"loss_config": "karras", "loss_weighting": "soft-min-snr", "dropout_rate": [0.0], "augment_prob": 0.0,
                            "sigma_sample_density": {"type": "cosine-interpolated"}})
    config.update({"dataset": {"type": "imagefolder", "location": str(data_dir)},
                   "optimizer": {"type": "adamw", "lr": 5e-4, "betas": [0.9, 0.95], "eps": 1e-8, "weight_decay": 1e-3},
                   "lr_sched": {"type": "constant", "warmup": 0.0}, "ema_sched": {"type": "inverse", "power": 0.75, "max_value": 0.9999}})
    (tmp_path / "config.json").write_text(json.dumps(config))
    common = ["--config", str(tmp_path / "config.json"), "--batch-size", "4", "--save-every", "100", "--demo-every", "100", "--seed", "1",
              "--num-workers", "0", "--end-step", "2", "--name", "run"]
    ckpt = {}
    for tag, extra in (("fp32", []), ("bf16", ["--mixed-precision", "bf16"])):
        (tmp_path / tag).mkdir()
        out = _run_train(tmp_path / tag, [*common, *extra])
        assert ("Mixed precision bf16" in out.stdout) == bool(extra), out.stdout[-1000:]
        ckpt[tag] = torch.load(tmp_path / tag / "run_00000002.pth", map_location="cpu", weights_only=False)
    assert ckpt["fp32"]["step"] == ckpt["bf16"]["step"] == 2
    a, b = ckpt["fp32"]["model"], ckpt["bf16"]["model"]
    assert a.keys() == b.keys() and not all(torch.equal(a[k], b[k]) for k in a)

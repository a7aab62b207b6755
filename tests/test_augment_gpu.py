"""Karras augmentation on the MI355X (csrc/augment_f32.hip, K.augmentation): the warp, cond and inverse-matrix kernels against the reference's
own matrices and conds (tests/golden/augment.json) and an fp64 restatement of the arithmetic (tests/augment_ref.py), the bit-exact and
reflect cases, the draw's contract and statistics, guard bands, the pipeline / wrapper surface and train.py --device-augment end to end.

Tolerances.  The kernel evaluates in fp32 what the restatement evaluates in fp64, so its bound is measured, per quantity and per input set, as
``base`` = the largest absolute difference between the SAME restatement run in fp32 torch and in fp64 on those inputs; the kernel is allowed
4 x base (reassociation, another libm).  Measured bases (CPU, deterministic): y 3.97e-6 ([4,3,16,16]), 5.00e-6 ([2,1,12,20]), 9.61e-6
([1,3,33,33]), 4.98e-7 ([3,2,2,5]) on images in [-1, 1]; cond 6.47e-8 (the 22 golden raws of either size); mat 3.70e-6 (16 x 16) and 3.05e-6
(20 x 12) against the fp64 inverse of the recorded fp32 matrix.  The integer-shift and one-hot cases have base 0: they are compared bit for bit.  Catmull-Rom is C1, so no pixel is
left out anywhere.
"""
import csv
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from k_diffusion_amd import _native as nat
from tests import augment_ref as ar
from tests.guard import Case, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 3, 16, 16), (2, 1, 12, 20), (1, 3, 33, 33), (3, 2, 2, 5)]
F32, F64 = torch.float32, torch.float64


def g(t):
    return t.to(DEV, F32).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def golden():
    return ar.load_golden()


def golden_raws(B, offset=0):
    """B raw rows of the golden file, cycled from ``offset`` (the raws do not depend on the image size)."""
    rows = [c["raw"] for c in golden()["cases"]]
    return torch.tensor([rows[(offset + i) % len(rows)] for i in range(B)], dtype=F32)


def images(shape, seed=5):
    return torch.rand(*shape, generator=_gen(seed)) * 2 - 1


@functools.lru_cache(maxsize=None)
def warp_reference(shape):
    """(x, raw, y64, base) of one shape: random images, golden raws, the fp64 restatement and the fp32-against-fp64 base.  Computed once."""
    B, _, H, W = shape
    x, raw = images(shape), golden_raws(B, offset=3 * H + W)
    y64 = ar.warp(x, ar.inverse_matrix(raw, H, W, dtype=F64))
    y32 = ar.warp(x, ar.inverse_matrix(raw, H, W, dtype=F32))
    return x, raw, y64, (y32.double() - y64).abs().max().item()


def within(got, ref64, base, what):
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: error {err:.3e}, base {base:.3e}, bound {4 * base:.3e}")
    assert err <= 4 * base, f"{what}: error {err:.3e} above 4 x base = {4 * base:.3e}"


# ---- 1. golden: the reference's own matrices and conds ----------------------------------------------------------------------------------

@pytest.mark.parametrize("width,height", [(16, 16), (20, 12)])
def test_golden_cond_and_matrix(KD, width, height):
    gd = golden()
    rows = [c for c in gd["cases"] if (c["width"], c["height"]) == (width, height)]
    assert len(rows) >= 19
    raw = torch.tensor([c["raw"] for c in rows], dtype=F32)
    x = images((len(rows), 1, height, width))
    _, cond, mat = KD.augmentation.augment_warp(g(x), g(raw), gd["a_scale"], gd["a_aniso"], gd["a_trans"], with_mat=True)
    rec_cond = torch.tensor([c["cond"] for c in rows], dtype=F64)
    base_cond = (ar.cond_of(raw, F32).double() - ar.cond_of(raw, F64)).abs().max().item()
    within(cond, rec_cond, base_cond, "cond")
    inv64 = torch.linalg.inv(torch.tensor([c["matrix"] for c in rows], dtype=F64))[:, :2].reshape(-1, 6)
    mat32 = ar.inverse_matrix(raw, height, width, gd["a_scale"], gd["a_aniso"], gd["a_trans"], dtype=F32)[:, :2].reshape(-1, 6)
    within(mat, inv64, (mat32.double() - inv64).abs().max().item(), "mat")


# ---- 2. the warp against the fp64 restatement -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_warp_matches_fp64_restatement(KD, shape):
    x, raw, y64, base = warp_reference(shape)
    assert base > 0
    y, cond = KD.augmentation.augment_warp(g(x), g(raw))
    within(y, y64, base, f"y {list(shape)}")
    assert torch.equal(y, KD.augmentation.augment_warp(g(x), g(raw))[0])


# ---- 3. bit-exact cases -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_and_flips_are_bit_exact(KD, shape):
    x = g(images(shape, seed=9))
    B = shape[0]
    for hot, want in ((None, x), (0, x.flip(-1)), (1, x.flip(-2))):
        raw = torch.zeros(B, 8)
        if hot is not None:
            raw[:, hot] = 1.0
        y, cond, mat = KD.augmentation.augment_warp(x, g(raw), with_mat=True)
        assert torch.equal(y.view(torch.int32), want.contiguous().view(torch.int32)), f"one-hot a{hot}: not bit-identical"
        assert torch.equal(cond.cpu(), ar.cond_of(raw, F32))


# ---- 4. the reflect rule ----------------------------------------------------------------------------------------------------------------------

def _fold(i, n):
    """d c b | a b c d | c b a"""
    period = 2 * (n - 1)
    i %= period
    return i if i < n else period - i


def test_reflect_rule_on_integer_shifts(KD):
    shape = (3, 3, 16, 16)
    x = images(shape, seed=11)
    raw = torch.zeros(3, 8)
    raw[0, 6], raw[1, 6], raw[2, 7] = 1.0, 12.0, -9.0            # a_trans * 16 = 2: shifts of 2 and 24 columns, -18 rows
    want = torch.stack([x[0][:, :, [_fold(c - 2, 16) for c in range(16)]], x[1][:, :, [_fold(c - 24, 16) for c in range(16)]],
                        x[2][:, [_fold(r + 18, 16) for r in range(16)], :]])
    y64 = ar.warp(x, ar.inverse_matrix(raw, 16, 16, a_trans=1 / 8, dtype=F64))
    y32 = ar.warp(x, ar.inverse_matrix(raw, 16, 16, a_trans=1 / 8, dtype=F32))
    assert torch.equal(y64, want.double())                       # the restatement agrees with the plain index gather
    base = (y32.double() - y64).abs().max().item()               # 0: every coordinate is an integer in fp32 too
    y, _ = KD.augmentation.augment_warp(g(x), g(raw), a_trans=1 / 8)
    within(y, want.double(), base, "integer shifts")


# ---- 5. the draw ------------------------------------------------------------------------------------------------------------------------------

def _key(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def test_draw_contract_and_statistics(KD):
    B, p = 4096, 0.5
    draw = KD.augmentation.augment_draw
    raw = draw(_key(1234567), B, p)
    assert torch.equal(raw, draw(_key(1234567), B, p))
    assert not torch.equal(raw, draw(_key(1234568), B, p))
    a = raw.cpu().double()
    # the contract restated (Philox words exact; the hardware log2 / sqrt / cos within the 1e-4 of oracle/brownian.py)
    ref, _ = ar.draw(1234567, B, p)
    assert np.array_equal(ref == 0, a.numpy() == 0)
    assert np.abs(ref - a.numpy()).max() < 1e-4, np.abs(ref - a.numpy()).max()
    assert np.array_equal(ref[:, [0, 1, 3, 4]], raw.cpu().numpy()[:, [0, 1, 3, 4]])          # bits and angles: the same fp32 arithmetic
    sigma = math.sqrt(p * (1 - p) / B)
    assert set(a[:, 0].unique().tolist()) <= {0.0, 1.0} and set(a[:, 1].unique().tolist()) <= {0.0, 1.0}
    assert abs((a[:, 0] == 1).double().mean().item() - 0.5) < 5 * math.sqrt(0.25 / B)
    assert abs((a[:, 1] == 1).double().mean().item() - p / 2) < 5 * math.sqrt(p / 2 * (1 - p / 2) / B)   # gate and bit independent
    fired = {k: a[:, k] != 0 for k in range(2, 8)}
    for k in (2, 3, 4, 6):
        assert abs(fired[k].double().mean().item() - p) < 5 * sigma, (k, fired[k].double().mean().item())
    assert torch.equal(fired[4], fired[5]) and torch.equal(fired[6], fired[7])
    for k, l in ((2, 3), (3, 4), (4, 6), (2, 6)):                # separate gates do not fire together
        assert not torch.equal(fired[k], fired[l])
    for k in (3, 4):
        assert (a[:, k] >= -math.pi).all() and (a[:, k] < math.pi).all()
    z = a[:, 2][fired[2]]
    n = z.numel()
    assert abs(z.mean().item()) < 5 / math.sqrt(n) and abs(z.var().item() - 1) < 5 * math.sqrt(2 / n), (z.mean().item(), z.var().item())
    none = draw(_key(99), B, 0.0).cpu()
    assert (none[:, 1:] == 0).all() and 0 < none[:, 0].sum() < B
    every = draw(_key(99), B, 1.0).cpu()
    assert (every[:, 2:] != 0).all() and 0 < every[:, 1].sum() < B
    assert torch.equal(none[:, 0], every[:, 0])                  # a0 does not depend on a_prob


# ---- 6. pipeline and wrapper ------------------------------------------------------------------------------------------------------------------

def test_pipeline_surface(KD):
    from PIL import Image
    aug = KD.augmentation.KarrasAugmentationPipeline(a_prob=0.5)
    assert (aug.a_prob, aug.a_scale, aug.a_aniso, aug.a_trans, aug.disable_all) == (0.5, 2 ** 0.2, 2 ** 0.2, 1 / 8, False)
    x = g(images((4, 3, 16, 16), seed=3))
    torch.manual_seed(21)
    image, orig, cond = aug.batch(x)
    assert orig is x and image.shape == x.shape and cond.shape == (4, 9) and not torch.equal(image, x)
    torch.manual_seed(21)
    again = aug.batch(x)
    assert torch.equal(again[0], image) and torch.equal(again[2], cond)
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = aug.batch(x, generator=gen)
    b = aug.batch(x, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    raw = g(golden_raws(4))
    given = aug.batch(x, raw=raw)
    y, c = KD.augmentation.augment_warp(x, raw)
    assert torch.equal(given[0], y) and torch.equal(given[2], c)
    off = KD.augmentation.KarrasAugmentationPipeline(disable_all=True).batch(x)
    assert off[0] is x and off[1] is x and torch.equal(off[2], torch.zeros(4, 9, device=DEV))
    # __call__: the per-image form over batch with B = 1
    arr = (torch.rand(12, 20, 3, generator=_gen(4)) * 255).to(torch.uint8).numpy()
    pil = Image.fromarray(arr, mode="RGB")
    torch.manual_seed(33)
    one = aug(pil)
    torch.manual_seed(33)
    ref = aug.batch(g(KD.utils.from_pil_image(pil).unsqueeze(0)))
    assert one[0].shape == (3, 12, 20) and one[2].shape == (9,) and one[0].is_cuda
    assert all(torch.equal(u, v[0]) for u, v in zip(one, ref))
    with pytest.raises(RuntimeError, match="ROCm device"):
        aug.batch(x.cpu())
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        aug.batch(g(torch.zeros(2, 3, 1, 8)))
    with pytest.raises(RuntimeError, match="overlap"):
        KD.augmentation.augment_warp(x, raw, out=x)


def test_loss_takes_the_cond(KD):
    from tests.test_likelihood_gpu import build
    from tests.test_param_grad_gpu import _inputs
    cfg, model, _ = build(KD, "tiny_sw")
    x, noise, sigma, kw = _inputs(cfg, 2)
    kw = {k: v.to(DEV) for k, v in kw.items() if k != "aug_cond"}
    aug = KD.augmentation.KarrasAugmentationPipeline(a_prob=1.0)
    torch.manual_seed(2)
    image, _, cond = aug.batch(g(x))
    den = KD.Denoiser(model, cfg["model"]["sigma_data"])
    with torch.no_grad():
        with_cond = den.loss(image, g(noise), g(sigma), aug_cond=cond, **kw)
        without = den.loss(image, g(noise), g(sigma), aug_cond=torch.zeros_like(cond), **kw)
    assert torch.isfinite(with_cond).all() and not torch.equal(with_cond, without)


# ---- 7. guard bands ---------------------------------------------------------------------------------------------------------------------------

def _warp_case(shape):
    def make(env):
        x, raw, y64, base = warp_reference(shape)
        B, Cn, H, W = shape

        def call(T):
            nat.check(nat.lib().kd_augment_warp_f32(T["x"].data_ptr(), T["raw"].data_ptr(), ar.A_SCALE, ar.A_ANISO, ar.A_TRANS, T["y"].data_ptr(),
                                                    T["cond"].data_ptr(), T["mat"].data_ptr(), B, Cn, H, W,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "kd_augment_warp_f32")
            return T["y"], T["cond"], T["mat"]
        cond64, mat64 = ar.cond_of(raw, F64), ar.inverse_matrix(raw, H, W, dtype=F64)[:, :2].reshape(B, 6)
        # y: the bound of test 2.  cond and mat (a handful of rows: too few for a measured base) from the format: cond entries are one or two
        # fp32 operations on values below 4, 4 ulp(4) = 2e-6; mat entries stay below 128 after about ten roundings, 10 ulp(64) = 8e-5
        return dict(ins={"x": x, "raw": raw}, outs={"y": (shape, F32), "cond": ((B, 9), F32), "mat": ((B, 6), F32)}, call=call,
                    ref=lambda R: (y64, cond64, mat64), tol=[("abs", 4 * base), ("abs", 2e-6), ("abs", 8e-5)])
    return Case(f"augment_warp{list(shape)}", "augment_warp", "augment_f32.hip", make, kernel="augment_warp_f32")


def _draw_case(B):
    def make(env):
        def call(T):
            nat.check(nat.lib().kd_augment_draw_f32(T["key"].data_ptr(), B, 0.5, T["raw"].data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "kd_augment_draw_f32")
            return T["raw"]
        return dict(ins={"key": torch.tensor([-77123], dtype=torch.int64)}, outs={"raw": ((B, 8), F32)}, call=call,
                    ref=lambda R: torch.from_numpy(ar.draw(-77123, B, 0.5)[0]), tol=("abs", 1e-4))
    return Case(f"augment_draw[B{B}]", "augment_draw", "augment_f32.hip", make, kernel="augment_draw_f32")


GUARD_CASES = [_warp_case(s) for s in SHAPES] + [_draw_case(B) for B in (1, 3, 300)]


@pytest.mark.parametrize("c", GUARD_CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")


# ---- 8. train.py --device-augment end to end --------------------------------------------------------------------------------------------------

def _run_train(cwd, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


def _losses(path):
    return [row["loss"] for row in csv.DictReader(open(path))]


def test_train_py_device_augment_end_to_end(KD, tmp_path):
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
                        "loss_config": "karras", "loss_weighting": "soft-min-snr", "dropout_rate": [0.0, 0.0], "augment_prob": 0.5,
                        "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80, "sigma_sample_density": {"type": "cosine-interpolated"}},
              "dataset": {"type": "imagefolder", "location": str(data_dir)},
              "optimizer": {"type": "adamw", "lr": 5e-4, "betas": [0.9, 0.95], "eps": 1e-8, "weight_decay": 1e-3},
              "lr_sched": {"type": "constant", "warmup": 0.0}, "ema_sched": {"type": "inverse", "power": 0.75, "max_value": 0.9999}}
    (tmp_path / "config.json").write_text(json.dumps(config))
    config["model"]["augment_prob"] = 0.0
    (tmp_path / "config0.json").write_text(json.dumps(config))
    common = ["--batch-size", "4", "--save-every", "2", "--demo-every", "1000", "--seed", "1", "--num-workers", "0", "--end-step", "4", "--name", "run",
              "--device-augment"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    out = _run_train(a, ["--config", str(tmp_path / "config.json"), *common])
    assert "Device augmentation" in out.stdout and (a / "run_00000002.pth").exists() and (a / "run_00000004.pth").exists()
    assert len(_losses(a / "run_log.csv")) == 4
    _run_train(b, ["--config", str(tmp_path / "config.json"), *common, "--resume", str(a / "run_00000002.pth")])
    full = torch.load(a / "run_00000004.pth", map_location="cpu", weights_only=False)
    resumed = torch.load(b / "run_00000004.pth", map_location="cpu", weights_only=False)
    for key in ("model", "model_ema"):
        assert full[key].keys() == resumed[key].keys()
        assert all(torch.equal(full[key][k], resumed[key][k]) for k in full[key]), key
    assert full["opt"]["state"].keys() == resumed["opt"]["state"].keys() and len(full["opt"]["state"]) > 0
    for i, st in full["opt"]["state"].items():
        assert all(torch.equal(st[k], resumed["opt"]["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq")), i
    out0 = _run_train(c, ["--config", str(tmp_path / "config0.json"), *common])
    assert "Device augmentation" not in out0.stdout
    assert _losses(a / "run_log.csv") != _losses(c / "run_log.csv")

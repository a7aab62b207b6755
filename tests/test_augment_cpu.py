"""Karras augmentation without a GPU: the library's two entry points and their signatures, the golden file against the fp64 restatement
(tests/augment_ref.py), the reference's wrapper on a CPU dummy model, the restated draw's invariants, and train.py's --device-augment flag."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import torch

from tests import augment_ref as ar
from tests.golden import cases
from tests.test_host_cpu import header_prototypes

F32, F64 = torch.float32, torch.float64


def test_library_exports_the_entry_points(KD):
    nat = KD._native
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert nat.SIGNATURES["kd_augment_draw_f32"] == [vp, i, f, vp, vp]
    assert nat.SIGNATURES["kd_augment_warp_f32"] == [vp, vp, f, f, f, vp, vp, vp, i, i, i, i, vp]
    protos = header_prototypes()
    assert protos["kd_augment_draw_f32"] == 5 and protos["kd_augment_warp_f32"] == 13
    handle = ctypes.CDLL(nat.LIB_PATH)
    assert hasattr(handle, "kd_augment_draw_f32") and hasattr(handle, "kd_augment_warp_f32")
    header = open(os.path.join(cases.REPO, "include", "kdiff_hip.h")).read()
    assert header.count("augmentation.py:40-89") >= 1 and "Counter contract" in header
    # the guards answer before any launch: no device needed
    lib = nat.lib()
    assert lib.kd_augment_warp_f32(1, 1, 1.1, 1.1, 0.1, 2, 1, None, 1, 1, 1, 8, None) != 0 and b"H, W >= 2" in lib.kd_last_error()
    assert lib.kd_augment_warp_f32(4096, 1, 1.1, 1.1, 0.1, 4096 + 64, 1, None, 1, 1, 8, 8, None) != 0 and b"overlap" in lib.kd_last_error()
    assert lib.kd_augment_draw_f32(1, 4, 1.5, 1, None) != 0 and b"a_prob" in lib.kd_last_error()
    assert KD.augmentation.KarrasAugmentationPipeline is not None and KD.augmentation.KarrasAugmentWrapper is not None


def test_golden_is_self_consistent():
    gd = ar.load_golden()
    assert (gd["a_scale"], gd["a_aniso"], gd["a_trans"]) == (2 ** 0.2, 2 ** 0.2, 1 / 8)
    sizes = {(c["width"], c["height"]) for c in gd["cases"]}
    assert sizes == {(16, 16), (20, 12)}
    assert sum(c["a_prob"] == 1.0 for c in gd["cases"]) >= 32 and sum(c["a_prob"] == 0.12 for c in gd["cases"]) >= 6
    for c in gd["cases"]:
        raw = torch.tensor([c["raw"]], dtype=F32)
        H, W = c["height"], c["width"]
        rec = torch.tensor(c["matrix"], dtype=F64)
        M = ar.forward_matrix(raw, H, W, gd["a_scale"], gd["a_aniso"], gd["a_trans"])[0]
        # the reference multiplies ten fp32 matrices with entries up to ~ W: ten roundings of ulp(32) = 3.8e-6 at the most
        assert (M - rec).abs().max() < 2e-5, (c["seed"], (M - rec).abs().max())
        assert torch.equal(rec[2], torch.tensor([0.0, 0.0, 1.0], dtype=F64))
        # cond: one or two fp32 operations on values below 4
        assert (ar.cond_of(raw)[0] - torch.tensor(c["cond"], dtype=F64)).abs().max() < 5e-7
        # the analytic inverse is the inverse
        Mi = ar.inverse_matrix(raw, H, W, gd["a_scale"], gd["a_aniso"], gd["a_trans"])[0]
        assert (Mi @ M - torch.eye(3, dtype=F64)).abs().max() < 1e-12
        if c["a_prob"] == 1.0:
            assert all(v != 0 for v in c["raw"][2:])
        assert c["raw"][0] in (0.0, 1.0) and c["raw"][1] in (0.0, 1.0)
        assert -math.pi <= c["raw"][3] < math.pi and -math.pi <= c["raw"][4] < math.pi


def test_restated_warp_rules():
    """The restatement the GPU tests lean on: zero raws give the identity, integer shifts follow the d c b | a b c d | c b a fold, and the
    interpolant reproduces linear ramps away from the fold."""
    x = torch.rand(2, 2, 6, 7, generator=torch.Generator().manual_seed(1), dtype=F64)
    assert torch.equal(ar.warp(x, ar.inverse_matrix(torch.zeros(2, 8), 6, 7)), x)
    assert ar.reflect(torch.tensor([-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]), 4).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert ar.reflect(torch.tensor([-3, -2, -1, 0, 1, 2, 3]), 2).tolist() == [1, 0, 1, 0, 1, 0, 1]
    ramp = torch.arange(12, dtype=F64).view(1, 1, 1, 12).expand(1, 1, 5, 12).contiguous()
    m = torch.eye(3, dtype=F64).unsqueeze(0).clone()
    m[0, 0, 2] = 0.25                                           # sample a quarter pixel to the right
    out = ar.warp(ramp, m)
    assert torch.allclose(out[0, 0, :, 1:10], ramp[0, 0, :, 1:10] + 0.25, atol=1e-12)


def test_restated_draw_invariants():
    raw, gates = ar.draw(42, 2048, 0.5)
    again, _ = ar.draw(42, 2048, 0.5)
    assert np.array_equal(raw, again) and not np.array_equal(raw, ar.draw(43, 2048, 0.5)[0])
    assert np.array_equal(raw[:, 4] != 0, gates[:, 3]) and np.array_equal(raw[:, 5] != 0, gates[:, 3])
    assert np.array_equal(raw[:, 6] != 0, gates[:, 4]) and np.array_equal(raw[:, 7] != 0, gates[:, 4])
    assert ((raw[:, 3] >= -math.pi) & (raw[:, 3] < math.pi)).all()
    assert abs(gates.mean() - 0.5) < 5 * math.sqrt(0.25 / gates.size)
    # the angle's extremes stay inside [-pi, pi) in fp32
    lo, hi = (np.float32(0) - np.float32(0.5)) * np.float32(6.28318501), (np.float32(1 - 2.0 ** -24) - np.float32(0.5)) * np.float32(6.28318501)
    assert -math.pi <= float(lo) and float(hi) < math.pi


class _Inner(torch.nn.Module):
    def forward(self, input, sigma, mapping_cond=None, extra=None):
        self.seen = (mapping_cond, extra)
        return input * 2

    def param_groups(self, base_lr):
        return [{"params": [], "lr": base_lr}]

    def set_skip_stages(self, skip_stages):
        return ("skip", skip_stages)

    def set_patch_size(self, patch_size):
        return ("patch", patch_size)


def test_wrapper_concatenates_aug_cond_in_front(KD):
    inner = _Inner()
    wrap = KD.augmentation.KarrasAugmentWrapper(inner)
    assert wrap.inner_model is inner
    x, sigma = torch.randn(3, 1, 4, 4), torch.ones(3)
    aug, mc = torch.randn(3, 9), torch.randn(3, 5)
    assert torch.equal(wrap(x, sigma, aug_cond=aug, mapping_cond=mc, extra=7), x * 2)
    assert torch.equal(inner.seen[0], torch.cat([aug, mc], dim=1)) and inner.seen[1] == 7
    wrap(x, sigma, aug_cond=aug)
    assert torch.equal(inner.seen[0], aug)
    wrap(x, sigma)
    assert inner.seen[0].shape == (3, 9) and not inner.seen[0].any() and inner.seen[0].dtype == x.dtype
    wrap(x, sigma, mapping_cond=mc)
    assert torch.equal(inner.seen[0], torch.cat([torch.zeros(3, 9), mc], dim=1))
    assert wrap.param_groups(1e-3) == [{"params": [], "lr": 1e-3}]
    assert wrap.set_skip_stages(1) == ("skip", 1) and wrap.set_patch_size(4) == ("patch", 4)


def test_pipeline_refuses_the_cpu(KD):
    import pytest
    aug = KD.augmentation.KarrasAugmentationPipeline()
    assert (aug.a_prob, aug.a_scale, aug.a_aniso, aug.a_trans, aug.disable_all) == (0.12, 2 ** 0.2, 2 ** 0.2, 1 / 8, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.batch(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KarrasOff = KD.augmentation.KarrasAugmentationPipeline(disable_all=True)
        KarrasOff.batch(torch.zeros(2, 3, 8, 8))


def test_train_py_device_augment_flag(KD):
    train = os.path.join(cases.REPO, "train.py")
    env = dict(os.environ, PYTHONPATH=cases.REPO)
    out = subprocess.run([sys.executable, train, "--device-augment", "--config", "none.json"], capture_output=True, text=True, env=env)
    assert out.returncode not in (0, 2) and "none.json" in out.stderr, out.stderr[-500:]      # past the parser: the config is missing
    assert "--device-augment" in subprocess.run([sys.executable, train, "--help"], capture_output=True, text=True, env=env).stdout

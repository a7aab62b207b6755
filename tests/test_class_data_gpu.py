"""Class-conditional data on the MI355X (csrc/data_u8.hip, K.data): the batch gather from a resident uint8 dataset and the conditioning
dropout, both bit for bit -- the gather against torch's own ``data[idx].float() / 255 * 2 - 1`` on the CPU, the dropout against the counter
contract of include/kdiff_hip.h restated with the oracle's Philox (integer arithmetic and one fp32 compare: no tolerance anywhere) -- guard
bands on both entry points, and train.py on a synthetic CIFAR-format dataset end to end.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from k_diffusion_amd import _native as nat
from oracle import brownian as obrown
from tests.guard import Case, run_case
from tests.test_class_data_cpu import _config, write_cifar

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 3, 5, 7), (5, 1, 28, 28), (4, 3, 32, 32)]          # 105 bytes per image: every odd index starts unaligned; MNIST; CIFAR
NUM_CLASSES = 10
COND_DROP_NODE = (1 << 63) | (1 << 62) | (1 << 32)


@functools.lru_cache(maxsize=None)
def dataset(shape):
    """(data uint8 [N, C, H, W] holding all 256 byte values, labels int64 [N], the whole set converted on the CPU by torch).  Computed once."""
    n = int(np.prod(shape))
    data = ((torch.arange(n) * 37 + 11) % 256).to(torch.uint8).reshape(shape)
    assert len(set(data.flatten().tolist())) == 256
    labels = (torch.arange(shape[0]) * 3 + 1) % NUM_CLASSES
    return data, labels, data.float() / 255 * 2 - 1


def index_sets(N):
    return [[0], [N - 1], [0, N - 1, 1, 1, N - 1, N // 2, 0, 3 % N, 1]]


def dropped(key, B, rate):
    """The rule of include/kdiff_hip.h: sample b is dropped iff u(w0) < rate in fp32, w0 = word 0 of philox4x32_10(key, (b, 2^63 | 2^62 | 2^32))."""
    w0 = obrown._philox(int(key) & (2 ** 64 - 1), np.arange(B, dtype=np.uint64), COND_DROP_NODE)[0]
    return torch.from_numpy(obrown._unit24(w0) < np.float32(rate))


def expected_classes(labels, key, rate):
    return torch.where(dropped(key, labels.numel(), rate), torch.full_like(labels, NUM_CLASSES), labels)


def dkey(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# ---- 1. the gather ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_is_bit_exact(KD, shape):
    data, labels, full = dataset(shape)
    ds = KD.data.DeviceImageDataset(data, device=DEV)
    assert len(ds) == shape[0]
    for idx in index_sets(shape[0]):
        reals, cls = ds.batch(idx)
        assert cls is None and reals.dtype == torch.float32 and tuple(reals.shape) == (len(idx), *shape[1:])
        ref = data[idx].float() / 255 * 2 - 1
        assert torch.equal(reals.cpu(), ref), (shape, idx, int((reals.cpu() != ref).sum()))
        assert torch.equal(ref, full[idx])
        again, _ = ds.batch(torch.tensor(idx))                        # a CPU tensor of indices is the same call
        assert torch.equal(again, reals)


def test_gather_matches_from_pil_image(KD):
    """The stated bits are those of utils.from_pil_image on the same bytes (a CIFAR row is planar, a PIL image interleaved)."""
    from PIL import Image
    data, _, _ = dataset((4, 3, 32, 32))
    reals, _ = KD.data.DeviceImageDataset(data, device=DEV).batch([2])
    pil = Image.fromarray(data[2].permute(1, 2, 0).contiguous().numpy(), mode="RGB")
    assert torch.equal(reals[0].cpu(), KD.utils.from_pil_image(pil))


# ---- 2. the dropout -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 5, 1000])
def test_dropout_is_bit_exact(KD, B):
    labels = (torch.arange(B) * 7 + 2) % NUM_CLASSES
    dl = labels.to(DEV)
    for key in (-77123, 2 ** 62 + 12345):
        for rate in (0.0, 0.1, 0.5, 1.0):
            got = KD.data.class_dropout(dl, dkey(key), rate, NUM_CLASSES)
            assert got.dtype == torch.int64 and torch.equal(dl.cpu(), labels)                  # the input is left alone
            assert torch.equal(got.cpu(), expected_classes(labels, key, rate)), (B, key, rate)
            assert torch.equal(KD.data.class_dropout(dl, dkey(key), rate, NUM_CLASSES), got)   # the same key gives the same bits
            if rate == 0.0:
                assert torch.equal(got.cpu(), labels)
                assert torch.equal(KD.data.class_dropout(dl, None, 0.0, NUM_CLASSES).cpu(), labels)
            if rate == 1.0:
                assert torch.equal(got.cpu(), torch.full_like(labels, NUM_CLASSES))
    inplace = dl.clone()
    assert KD.data.class_dropout(inplace, dkey(5), 0.5, NUM_CLASSES, out=inplace) is inplace
    assert torch.equal(inplace.cpu(), expected_classes(labels, 5, 0.5))
    if B == 1000:
        a, b = (KD.data.class_dropout(dl, dkey(k), 0.5, NUM_CLASSES).cpu() for k in (-77123, -77122))
        assert not torch.equal(a, b)
        n = int((a == NUM_CLASSES).sum())
        assert 400 < n < 600, n                   # Bernoulli(1/2) over 1000 samples: 6 sigma = 95


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_batch_equals_gather_then_dropout(KD, shape):
    data, labels, full = dataset(shape)
    ds = KD.data.DeviceImageDataset(data, labels, device=DEV, num_classes=NUM_CLASSES)
    plain = KD.data.DeviceImageDataset(data, device=DEV)
    for idx in index_sets(shape[0]):
        for rate in (0.0, 0.5, 1.0):
            key = dkey(991 + len(idx))
            reals, cls = ds.batch(idx, key, rate, NUM_CLASSES)
            assert torch.equal(reals, plain.batch(idx)[0]) and torch.equal(reals.cpu(), full[idx])
            two_step = KD.data.class_dropout(labels[idx].to(DEV), key, rate, NUM_CLASSES)
            assert cls.dtype == torch.int64 and torch.equal(cls, two_step), (shape, idx, rate)
            assert torch.equal(cls.cpu(), expected_classes(labels[idx], 991 + len(idx), rate))
    reals, cls = ds.batch([1, 0])                                     # num_classes 0: the labels are ignored
    assert cls is None
    with pytest.raises(ValueError, match="needs a key"):
        ds.batch([1, 0], None, 0.1, NUM_CLASSES)
    with pytest.raises(IndexError, match="outside"):
        ds.batch([shape[0]], dkey(1), 0.1, NUM_CLASSES)


# ---- 3. guard bands -----------------------------------------------------------------------------------------------------------------------------

def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch_case(shape, idx, labelled):
    def make(env):
        data, labels, full = dataset(shape)
        B, (_, Cn, H, W) = len(idx), shape
        key, rate = 424242, 0.5
        ins = {"data": data, "idx": torch.tensor(idx)}
        outs = {"out": ((B, Cn, H, W), torch.float32)}
        if labelled:
            ins.update(labels=labels, key=torch.tensor([key]))
            outs["class_out"] = ((B,), torch.int64)

        def call(T):
            opt = {k: T[k].data_ptr() if labelled else None for k in ("labels", "key", "class_out")}
            nat.check(nat.lib().kd_batch_u8_f32(T["data"].data_ptr(), opt["labels"], T["idx"].data_ptr(), opt["key"], rate, NUM_CLASSES,
                                                T["out"].data_ptr(), opt["class_out"], B, Cn, H, W, _stream()), "kd_batch_u8_f32")
            return (T["out"], T["class_out"]) if labelled else T["out"]

        def ref(R):
            x = R["data"][R["idx"]].float() / 255 * 2 - 1
            return (x, expected_classes(R["labels"][R["idx"]], key, rate)) if labelled else x
        return dict(ins=ins, outs=outs, call=call, ref=ref, ref32=True, tol=0)
    return Case(f"batch_u8{list(shape)}[B{len(idx)}{',labels' if labelled else ''}]", "batch_u8", "data_u8.hip", make, kernel="batch_u8_f32")


def _dropout_case(B):
    def make(env):
        labels = (torch.arange(B) * 3 + 1) % NUM_CLASSES
        key, rate = -99, 0.5

        def call(T):
            nat.check(nat.lib().kd_class_dropout_i64(T["labels"].data_ptr(), T["key"].data_ptr(), rate, NUM_CLASSES, T["out"].data_ptr(), B, _stream()),
                      "kd_class_dropout_i64")
            return T["out"]
        return dict(ins={"labels": labels, "key": torch.tensor([key])}, outs={"out": ((B,), torch.int64)}, call=call,
                    ref=lambda R: expected_classes(R["labels"], key, rate), ref32=True, tol=0)
    return Case(f"class_dropout[B{B}]", "class_dropout", "data_u8.hip", make, kernel="class_dropout_i64")


GUARD_CASES = [_batch_case((7, 3, 5, 7), index_sets(7)[2], True), _batch_case((7, 3, 5, 7), index_sets(7)[2], False), _dropout_case(5)]


@pytest.mark.parametrize("c", GUARD_CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    assert all(e == 0.0 for e in res.errs)


# ---- 4. train.py on a resident labelled dataset, end to end ------------------------------------------------------------------------------------

def _run_train(cwd, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


def _start_weights(KD, cfg, path):
    """An inference checkpoint of synthetic NON-ZERO weights for ``train.py --resume-inference``.  A freshly initialised HDiT cannot show
    what these tests look for within four steps: patch_out, every out_proj / down_proj and every AdaRMSNorm projection start at zero
    (the reference's zero_init), so the gradient of the class table is EXACTLY zero until the fourth optimizer step -- one step each to
    open the output projection, the block projections and the norm projections.  From non-zero weights it is non-zero at once."""
    from safetensors.torch import save_file
    model = KD.config.make_model(KD.config.load_config(cfg))
    save_file(KD.synth.synth_state_dict(model.state_dict(), seed=7), str(path))
    return str(path)


def _emb(path):
    return torch.load(path, map_location="cpu", weights_only=False)["model"]["class_emb.weight"]


def test_train_py_class_conditional_end_to_end(KD, tmp_path):
    """(A) cond_dropout_rate 1: every sample carries the extra id, so rows 0 .. 9 of the class table see a zero gradient and -- without weight
    decay -- AdamW leaves their bits alone, while row 10 trains.  (B) rate 0: the other way round, and the CFG demo runs.  (C) a resume from
    B's middle checkpoint ends bit for bit where B ended.  A and B start from synthetic non-zero weights (``_start_weights``)."""
    from PIL import Image
    write_cifar(tmp_path / "data")                                    # 5 files x 4 rows = 20 images
    for tag, rate in (("a", 1.0), ("b", 0.0)):
        cfg = _config({"type": "cifar10", "location": str(tmp_path / "data"), "num_classes": NUM_CLASSES, "cond_dropout_rate": rate})
        (tmp_path / f"config_{tag}.json").write_text(json.dumps(cfg))
    start = ["--resume-inference", _start_weights(KD, cfg, tmp_path / "start.safetensors")]
    common = ["--batch-size", "4", "--grad-accum-steps", "2", "--save-every", "2", "--end-step", "4", "--sample-n", "4", "--seed", "1", "--name", "run"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()

    out = _run_train(a, ["--config", str(tmp_path / "config_a.json"), *common, *start, "--demo-every", "1000"])
    assert "resident on the device" in out.stdout and "Number of items in dataset: 20" in out.stdout
    e2, e4 = _emb(a / "run_00000002.pth"), _emb(a / "run_00000004.pth")
    assert tuple(e2.shape)[0] == NUM_CLASSES + 1
    assert torch.equal(e2[:NUM_CLASSES], e4[:NUM_CLASSES]) and not torch.equal(e2[NUM_CLASSES], e4[NUM_CLASSES])
    assert not list(a.glob("run_demo_*.png"))

    _run_train(b, ["--config", str(tmp_path / "config_b.json"), *common, *start, "--demo-every", "4"])
    e2, e4 = _emb(b / "run_00000002.pth"), _emb(b / "run_00000004.pth")
    assert torch.equal(e2[NUM_CLASSES], e4[NUM_CLASSES]) and not torch.equal(e2[:NUM_CLASSES], e4[:NUM_CLASSES])
    assert Image.open(b / "run_demo_00000004.png").size == (64, 64)

    _run_train(c, ["--config", str(tmp_path / "config_b.json"), *common, "--demo-every", "4", "--resume", str(b / "run_00000002.pth")])
    full = torch.load(b / "run_00000004.pth", map_location="cpu", weights_only=False)
    resumed = torch.load(c / "run_00000004.pth", map_location="cpu", weights_only=False)
    for key in ("model", "model_ema"):
        assert full[key].keys() == resumed[key].keys()
        assert all(torch.equal(full[key][k], resumed[key][k]) for k in full[key]), key
    assert full["opt"]["state"].keys() == resumed["opt"]["state"].keys() and len(full["opt"]["state"]) > 0
    for i, st in full["opt"]["state"].items():
        assert all(torch.equal(st[k], resumed["opt"]["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq")), i
    assert full["opt"]["param_groups"] == resumed["opt"]["param_groups"]


def test_train_py_class_folders_through_the_data_loader(KD, tmp_path):
    """``imagefolder-class``: the labels come through the DataLoader and are dropped by K.data.class_dropout.  At rate 1 only the extra row of
    the class table trains (from synthetic non-zero weights: ``_start_weights``)."""
    from PIL import Image
    gen = torch.Generator().manual_seed(8)
    for name in ("b", "c", "a"):
        (tmp_path / "images" / name).mkdir(parents=True)
        for i in range(4):
            arr = (torch.rand(32, 32, 3, generator=gen) * 255).to(torch.uint8).numpy()
            Image.fromarray(arr, mode="RGB").save(tmp_path / "images" / name / f"img_{i}.png")
    cfg = _config({"type": "imagefolder-class", "location": str(tmp_path / "images"), "num_classes": 3, "cond_dropout_rate": 1.0})
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    out = _run_train(tmp_path, ["--config", str(tmp_path / "config.json"), "--batch-size", "4", "--save-every", "1", "--end-step", "2", "--demo-every", "1000",
                                "--seed", "1", "--name", "run", "--num-workers", "0", "--resume-inference",
                                _start_weights(KD, cfg, tmp_path / "start.safetensors")])
    assert "Number of items in dataset: 12" in out.stdout and "resident" not in out.stdout
    e1, e2 = _emb(tmp_path / "run_00000001.pth"), _emb(tmp_path / "run_00000002.pth")
    assert tuple(e1.shape)[0] == 4
    assert torch.equal(e1[:3], e2[:3]) and not torch.equal(e1[3], e2[3])

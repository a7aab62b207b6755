"""Class-conditional data on the host (K.data, train.py's dataset checks), WITHOUT a GPU: the CIFAR-10 / MNIST file readers on synthetic
files in the formats torchvision leaves on disk, the class-folder dataset, the custom dataset loader, the argument refusals of the two C-ABI
entry points of csrc/data_u8.hip, and what train.py refuses before it asks for a device."""
import gzip
import json
import os
import pickle
import struct

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- readers ------------------------------------------------------------------------------------------------------------------------------------

def write_cifar(root, rows_per_file=4, seed=3):
    """Five pickles of ``rows_per_file`` rows each under root/cifar-10-batches-py; returns (uint8 [n, 3072], labels list) as written."""
    d = root / "cifar-10-batches-py"
    d.mkdir(parents=True)
    gen = _gen(seed)
    rows, labels = [], []
    for i in range(1, 6):
        data = torch.randint(0, 256, (rows_per_file, 3072), generator=gen, dtype=torch.uint8).numpy()
        lab = torch.randint(0, 10, (rows_per_file,), generator=gen).tolist()
        with open(d / f"data_batch_{i}", "wb") as f:
            pickle.dump({"batch_label": f"training batch {i} of 5", "labels": lab, "data": data, "filenames": [f"{i}_{j}.png" for j in range(rows_per_file)]}, f,
                        protocol=2)
        rows.append(data)
        labels += lab
    return np.concatenate(rows), labels


def idx_bytes(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    return struct.pack(">BBBB", 0, 0, 8, arr.ndim) + struct.pack(">" + "I" * arr.ndim, *arr.shape) + arr.tobytes()


def write_mnist(root, n=6, seed=4, gz=False):
    d = root / "MNIST" / "raw"
    d.mkdir(parents=True)
    gen = _gen(seed)
    images = torch.randint(0, 256, (n, 28, 28), generator=gen, dtype=torch.uint8).numpy()
    labels = torch.randint(0, 10, (n,), generator=gen, dtype=torch.uint8).numpy()
    for name, arr in (("train-images-idx3-ubyte", images), ("train-labels-idx1-ubyte", labels)):
        if gz:
            with gzip.open(d / (name + ".gz"), "wb") as f:
                f.write(idx_bytes(arr))
        else:
            (d / name).write_bytes(idx_bytes(arr))
    return images, labels


def test_read_cifar10_round_trips(KD, tmp_path):
    rows, labels = write_cifar(tmp_path)
    x, y = KD.data.read_cifar10(tmp_path)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (20, 3, 32, 32) and x.is_contiguous()
    assert y.dtype == torch.int64 and tuple(y.shape) == (20,)
    assert x.numpy().tobytes() == rows.tobytes()                  # planar: a row is the R, G and B planes in turn
    assert np.array_equal(x[7, 2].numpy(), rows[7, 2048:].reshape(32, 32))
    assert y.tolist() == labels


def test_read_cifar10_missing_file_names_the_path(KD, tmp_path):
    write_cifar(tmp_path)
    missing = tmp_path / "cifar-10-batches-py" / "data_batch_4"
    missing.unlink()
    with pytest.raises(FileNotFoundError) as e:
        KD.data.read_cifar10(tmp_path)
    assert str(missing) in str(e.value) and "must already be there" in str(e.value)


@pytest.mark.parametrize("gz", [False, True], ids=["raw", "gz-only"])
def test_read_mnist_round_trips(KD, tmp_path, gz):
    images, labels = write_mnist(tmp_path, gz=gz)
    x, y = KD.data.read_mnist(tmp_path)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (6, 1, 28, 28) and x.is_contiguous()
    assert y.dtype == torch.int64 and tuple(y.shape) == (6,)
    assert x.numpy().tobytes() == images.tobytes()
    assert y.tolist() == labels.tolist()


def test_read_mnist_missing_file_names_the_path(KD, tmp_path):
    write_mnist(tmp_path)
    missing = tmp_path / "MNIST" / "raw" / "train-labels-idx1-ubyte"
    missing.unlink()
    with pytest.raises(FileNotFoundError) as e:
        KD.data.read_mnist(tmp_path)
    assert str(missing) in str(e.value) and "must already be there" in str(e.value)
    with pytest.raises(FileNotFoundError, match="train-images-idx3-ubyte"):
        KD.data.read_mnist(tmp_path / "nowhere")


def test_read_mnist_refuses_a_wrong_header(KD, tmp_path):
    write_mnist(tmp_path)
    path = tmp_path / "MNIST" / "raw" / "train-images-idx3-ubyte"
    path.write_bytes(path.read_bytes()[:-1])                      # one byte short of what the header says
    with pytest.raises(ValueError, match="payload"):
        KD.data.read_mnist(tmp_path)


# ---- FolderOfImagesWithClasses --------------------------------------------------------------------------------------------------------------------

def _png(path, value):
    from PIL import Image
    Image.fromarray(np.full((4, 4, 3), value, dtype=np.uint8), mode="RGB").save(path)


def test_folder_of_images_with_classes(KD, tmp_path):
    root = tmp_path / "images"
    root.mkdir()
    counts = {"zebra": 2, "ant": 1, "mole": 3}                    # created in this (non-sorted) order
    for name, n in counts.items():
        (root / name).mkdir()
        for i in reversed(range(n)):
            _png(root / name / f"img_{i}.png", 40 * i + len(name))
    (root / "mole" / "notes.txt").write_text("not an image")
    (root / "stray.png").write_bytes(b"")                         # a file beside the class directories is no class
    ds = KD.data.FolderOfImagesWithClasses(root)
    assert ds.classes == ["ant", "mole", "zebra"]
    assert ds.class_to_idx == {"ant": 0, "mole": 1, "zebra": 2}
    assert len(ds) == 6
    assert [ds[i][1] for i in range(6)] == [0, 1, 1, 1, 2, 2]
    assert [p.name for p, _ in ds.samples] == ["img_0.png", "img_0.png", "img_1.png", "img_2.png", "img_0.png", "img_1.png"]
    image, label = ds[3]                                          # mole/img_2.png
    assert image.size == (4, 4) and image.getpixel((0, 0)) == (84, 84, 84) and label == 1
    with_tf = KD.data.FolderOfImagesWithClasses(root, transform=KD.utils.from_pil_image)
    x, label = with_tf[0]
    assert tuple(x.shape) == (3, 4, 4) and x.dtype == torch.float32 and label == 0


def test_folder_of_images_with_classes_refuses_an_empty_class(KD, tmp_path):
    root = tmp_path / "images"
    (root / "full").mkdir(parents=True)
    _png(root / "full" / "a.png", 1)
    (root / "empty").mkdir()
    (root / "empty" / "readme.txt").write_text("no image here")
    with pytest.raises(FileNotFoundError, match="empty"):
        KD.data.FolderOfImagesWithClasses(root)


# ---- load_custom --------------------------------------------------------------------------------------------------------------------------------

def test_load_custom(KD, tmp_path):
    (tmp_path / "sets").mkdir()
    (tmp_path / "sets" / "mine.py").write_text("def get_dataset(config, transform=None):\n    return [(transform(i), i % config['classes']) for i in range(config['n'])]\n")
    (tmp_path / "sets" / "other.py").write_text("def build(config, transform=None):\n    return ('other', config, transform)\n")
    cfg = tmp_path / "config.json"
    got = KD.data.load_custom(cfg, {"type": "custom", "location": "sets/mine.py", "config": {"n": 5, "classes": 2}}, lambda v: 10 * v)
    assert got == [(0, 0), (10, 1), (20, 0), (30, 1), (40, 0)]
    got = KD.data.load_custom(cfg, {"type": "custom", "location": "sets/other.py", "get_dataset": "build"}, None)
    assert got == ("other", {}, None)
    with pytest.raises(FileNotFoundError, match="absent.py"):
        KD.data.load_custom(cfg, {"type": "custom", "location": "sets/absent.py"}, None)


# ---- C ABI refusals -------------------------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_gpu(KD):
    """Argument validation happens before any launch (the pointers are never dereferenced on the host)."""
    lib = KD._native.lib()
    p = 4096                                                      # any non-NULL address
    ok = dict(data=p, labels=p, idx=p, key=p, rate=0.1, ncls=10, out=p, cout=p, B=4, C=3, H=5, W=7)

    def batch(**kw):
        a = dict(ok, **kw)
        return lib.kd_batch_u8_f32(a["data"], a["labels"], a["idx"], a["key"], a["rate"], a["ncls"], a["out"], a["cout"], a["B"], a["C"], a["H"], a["W"], None)
    for bad in (dict(data=None), dict(idx=None), dict(out=None), dict(B=0), dict(B=-1), dict(C=0), dict(H=0), dict(W=-3)):
        assert batch(**bad) == -1, bad
        assert b"kd_batch_u8_f32" in lib.kd_last_error()
    assert batch(labels=None) == -1 and b"go together" in lib.kd_last_error()           # class_out without labels
    assert batch(cout=None) == -1 and b"go together" in lib.kd_last_error()
    assert batch(key=None) == -1 and b"key" in lib.kd_last_error()
    assert batch(rate=1.5) == -1 and b"drop_rate" in lib.kd_last_error()
    assert batch(rate=float("nan")) == -1
    assert batch(ncls=0) == -1 and b"num_classes" in lib.kd_last_error()
    assert batch(C=1 << 12, H=1 << 10, W=1 << 10) == -1 and b"32-bit" in lib.kd_last_error()

    def drop(labels=p, key=p, rate=0.1, ncls=10, out=p, B=5):
        return lib.kd_class_dropout_i64(labels, key, rate, ncls, out, B, None)
    for bad in (dict(labels=None), dict(out=None), dict(B=0), dict(B=-2)):
        assert drop(**bad) == -1, bad
        assert b"kd_class_dropout_i64" in lib.kd_last_error()
    assert drop(key=None) == -1 and b"key" in lib.kd_last_error()
    assert drop(rate=-0.1) == -1 and b"drop_rate" in lib.kd_last_error()
    assert drop(ncls=0) == -1 and b"num_classes" in lib.kd_last_error()


def test_wrappers_have_no_cpu_fallback(KD):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.data.class_dropout(torch.zeros(3, dtype=torch.int64), None, 0.0, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.data.batch_u8(torch.zeros(2, 1, 4, 4, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))


def test_device_image_dataset_checks_on_the_host(KD):
    images = torch.zeros(4, 1, 3, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        KD.data.DeviceImageDataset(images.float(), device="cpu")
    with pytest.raises(ValueError, match="labels"):
        KD.data.DeviceImageDataset(images, torch.zeros(3, dtype=torch.int64), device="cpu")
    with pytest.raises(ValueError, match="outside"):
        KD.data.DeviceImageDataset(images, torch.tensor([0, 1, 10, 2]), device="cpu", num_classes=10)
    with pytest.raises(ValueError, match="outside"):
        KD.data.DeviceImageDataset(images, torch.tensor([0, -1, 3, 2]), device="cpu")
    ds = KD.data.DeviceImageDataset(images, torch.tensor([0, 1, 9, 2]), device="cpu", num_classes=10)
    assert len(ds) == 4
    for bad in ([4], [-1], [0, 1, 7]):
        with pytest.raises(IndexError, match="outside"):
            ds.batch(bad)
    with pytest.raises(ValueError, match="non-empty"):
        ds.batch([])
    with pytest.raises(ValueError, match="reach 9"):
        ds.batch([0], None, 0.0, 5)
    with pytest.raises(ValueError, match="no labels"):
        KD.data.DeviceImageDataset(images, device="cpu").batch([0], None, 0.0, 10)


# ---- train.py refusals ----------------------------------------------------------------------------------------------------------------------------

def _config(dataset, input_size=(32, 32), channels=3):
    return {"model": {"type": "image_transformer_v2", "input_channels": channels, "input_size": list(input_size), "patch_size": [4, 4], "depths": [1, 1],
                      "widths": [64, 128], "self_attns": [{"type": "shifted-window", "d_head": 64, "window_size": 4}, {"type": "global", "d_head": 64}],
                      "loss_config": "karras", "loss_weighting": "soft-min-snr", "dropout_rate": [0.0, 0.0], "augment_prob": 0.0,
                      "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80, "sigma_sample_density": {"type": "cosine-interpolated"}},
            "dataset": dataset,
            "optimizer": {"type": "adamw", "lr": 5e-4, "betas": [0.9, 0.95], "eps": 1e-8, "weight_decay": 0.0},
            "lr_sched": {"type": "constant", "warmup": 0.0}, "ema_sched": {"type": "inverse", "power": 0.75, "max_value": 0.9999}}


def _main(tmp_path, config):
    import train
    path = tmp_path / "config.json"
    path.write_text(json.dumps(config))
    return train.main(["--config", str(path), "--name", str(tmp_path / "run")])


def test_train_refuses_huggingface_by_name(tmp_path):
    with pytest.raises(NotImplementedError, match="huggingface"):
        _main(tmp_path, _config({"type": "huggingface", "location": "nowhere/at-all", "image_key": "image"}))


def test_train_refuses_mnist_at_another_size(tmp_path):
    with pytest.raises(NotImplementedError, match="native 28 x 28"):
        _main(tmp_path, _config({"type": "mnist", "location": str(tmp_path), "num_classes": 10}, input_size=(32, 32), channels=1))


def test_train_refuses_what_it_cannot_feed(KD, tmp_path):
    import train
    with pytest.raises(NotImplementedError, match="no class labels"):
        _main(tmp_path, _config({"type": "imagefolder", "location": str(tmp_path), "num_classes": 10}))
    with pytest.raises(ValueError, match="Invalid dataset type"):
        _main(tmp_path, _config({"type": "webdataset", "location": str(tmp_path)}))
    with pytest.raises(NotImplementedError, match="native 32 x 32"):
        _main(tmp_path, _config({"type": "cifar10", "location": str(tmp_path), "num_classes": 10}, input_size=(64, 64)))
    # the accepted types pass the checks (main would go on to ask for a device)
    for kind, size, ch in (("imagefolder", 16, 3), ("imagefolder-class", 16, 3), ("custom", 16, 3), ("cifar10", 32, 3), ("mnist", 28, 1)):
        cfg = KD.config.load_config(_config({"type": kind, "location": "x", "num_classes": 0 if kind == "imagefolder" else 10}, (size, size), ch))
        train.check_dataset_config(cfg)


def test_train_refuses_a_class_table_of_another_size(KD):
    import train
    cfg = KD.config.load_config(_config({"type": "cifar10", "location": "x", "num_classes": 10}))
    model = KD.config.make_model(cfg)
    assert model.num_classes == 11 and tuple(model.class_emb.weight.shape)[0] == 11
    train.check_dataset_config(cfg, model.num_classes)
    cfg["dataset"]["num_classes"] = 100                           # the config now disagrees with the model that was built
    with pytest.raises(ValueError, match="101 rows.*the model has 11"):
        train.check_dataset_config(cfg, model.num_classes)
    cfg["dataset"]["num_classes"] = 0
    with pytest.raises(ValueError, match="0 rows.*the model has 11"):
        train.check_dataset_config(cfg, model.num_classes)

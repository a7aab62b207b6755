"""Labelled training data: the dataset types of the reference's train.py (:203-225) other than ``imagefolder``, and the conditioning
dropout of its training step (:449-450), over this project's HIP kernels (csrc/data_u8.hip; arithmetic and counter contract:
include/kdiff_hip.h).

CIFAR-10 and MNIST are arrays, not image files: ``DeviceImageDataset`` keeps the whole uint8 training set in device memory and assembles a
step's batch -- the gather, the conversion to fp32 in [-1, 1] with the bits of ``utils.from_pil_image``, the labels and their dropout -- in
one launch.  There is no PIL round trip, no loader worker and no CPU path.  The dropped labels come from this project's counter-based
generator -- NOT the torch RNG stream of the reference.

The reference reaches these datasets through torchvision (``datasets.CIFAR10`` / ``datasets.MNIST`` / ``datasets.ImageFolder``).
torchvision is not a dependency here and none of it was available to record fixtures from: the file formats (``read_cifar10``,
``read_mnist``) and the class-folder rules (``FolderOfImagesWithClasses``) are restated from its documented behaviour.  Nothing is ever
downloaded: a missing file is an error.

``batch_u8`` / ``class_dropout`` are the tensor-level wrappers over the C ABI (the module's counterpart of ``ops``).
"""
import gzip
import importlib.util
import os
from pathlib import Path
import pickle
import struct

import torch

from . import _native as nat
from .ops import _chk, _p, _stream
from .utils import FolderOfImages


def _key(key, what, rate):
    """The call's key pointer: one int64 on the device, or None where nothing can be dropped."""
    if key is None:
        if rate > 0:
            raise ValueError(f"{what}: a drop rate of {rate:g} needs a key (a one-element int64 device tensor)")
        return None
    if _chk(key, "key", torch.int64).numel() != 1:
        raise ValueError(f"{what}: the key is one int64 (got {key.numel()} elements)")
    return key


def _rate(rate, num_classes, what):
    rate, num_classes = float(rate), int(num_classes)
    if not 0.0 <= rate <= 1.0:
        raise ValueError(f"{what}: the drop rate {rate:g} is outside [0, 1]")
    if num_classes <= 0:
        raise ValueError(f"{what}: num_classes must be positive (got {num_classes})")
    return rate, num_classes


def class_dropout(labels, key, rate, num_classes, out=None):
    """labels [B] int64 on the device -> the labels with sample b replaced by ``num_classes`` iff it is dropped: ``kd_class_dropout_i64``,
    the reference's train.py:449-450 on the counter contract of include/kdiff_hip.h.  ``key``: a one-element int64 device tensor (None is
    allowed at rate 0).  The same key gives the same bits.  ``out`` may be ``labels`` itself."""
    if _chk(labels, "labels", torch.int64).dim() != 1:
        raise ValueError(f"class_dropout: labels are [B] (got {tuple(labels.shape)})")
    rate, num_classes = _rate(rate, num_classes, "class_dropout")
    key = _key(key, "class_dropout", rate)
    out = torch.empty_like(labels) if out is None else out
    if _chk(out, "out", torch.int64).shape != labels.shape:
        raise ValueError(f"class_dropout: out shape {tuple(out.shape)} != {tuple(labels.shape)}")
    if labels.numel() == 0:
        return out
    nat.check(nat.lib().kd_class_dropout_i64(_p(labels), _p(key), rate, num_classes, _p(out), labels.numel(), _stream()), "kd_class_dropout_i64")
    return out


def batch_u8(data, idx, labels=None, key=None, rate=0., num_classes=0):
    """(out, class_out) for data [N, C, H, W] uint8 and idx [B] int64, both on the device: ``kd_batch_u8_f32``.  out [B, C, H, W] fp32 =
    ``data[idx].float() / 255 * 2 - 1`` bit for bit; with ``labels`` [N] int64, class_out [B] = ``labels[idx]`` after ``class_dropout``'s
    rule (else None).  Every idx must lie in [0, N): the kernel does not check (``DeviceImageDataset.batch`` does, on the host)."""
    if _chk(data, "data", torch.uint8).dim() != 4:
        raise ValueError(f"batch_u8: data is [N, C, H, W] (got {tuple(data.shape)})")
    if _chk(idx, "idx", torch.int64).dim() != 1 or idx.numel() == 0:
        raise ValueError(f"batch_u8: idx is [B], B >= 1 (got {tuple(idx.shape)})")
    N, C, H, W = data.shape
    B = idx.numel()
    out, class_out = torch.empty(B, C, H, W, device=data.device, dtype=torch.float32), None
    if labels is None:
        rate, num_classes = 0., 0
    else:
        if tuple(_chk(labels, "labels", torch.int64).shape) != (N,):
            raise ValueError(f"batch_u8: labels shape {tuple(labels.shape)} != {(N,)}")
        rate, num_classes = _rate(rate, num_classes, "batch_u8")
        key = _key(key, "batch_u8", rate)
        class_out = torch.empty(B, device=data.device, dtype=torch.int64)
    nat.check(nat.lib().kd_batch_u8_f32(_p(data), _p(labels), _p(idx), _p(key) if labels is not None else None, rate, num_classes, _p(out),
                                        _p(class_out), B, C, H, W, _stream()), "kd_batch_u8_f32")
    return out, class_out


class DeviceImageDataset:
    """A whole uint8 image dataset in device memory: ``images_u8`` [N, C, H, W] (planar) and, for a labelled one, ``labels`` [N] int64.
    ``batch`` assembles a training batch in one launch."""

    def __init__(self, images_u8, labels=None, device="cuda", num_classes=None):
        images_u8 = torch.as_tensor(images_u8)
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[0] == 0:
            raise ValueError(f"DeviceImageDataset: images are uint8 [N, C, H, W], N >= 1 (got {images_u8.dtype} {tuple(images_u8.shape)})")
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.dtype != torch.int64 or tuple(labels.shape) != (images_u8.shape[0],):
                raise ValueError(f"DeviceImageDataset: labels are int64 [{images_u8.shape[0]}] (got {labels.dtype} {tuple(labels.shape)})")
            lo, hi = int(labels.min()), int(labels.max())
            if lo < 0 or (num_classes is not None and hi >= num_classes):
                raise ValueError(f"DeviceImageDataset: labels span {lo} .. {hi}, outside [0, {num_classes if num_classes is not None else 'inf'})")
            self.max_label = hi
        self.n = images_u8.shape[0]
        self.images = images_u8.contiguous().to(device)
        self.labels = None if labels is None else labels.contiguous().to(device)

    def __len__(self):
        return self.n

    def __repr__(self):
        return f"DeviceImageDataset({tuple(self.images.shape)}, labels: {self.labels is not None}, device: {self.images.device})"

    def batch(self, indices, key=None, cond_dropout_rate=0., num_classes=0):
        """(reals fp32 [B, C, H, W], class_cond int64 [B] or None) for ``indices`` (a CPU int64 tensor or a list), range-checked here on the
        host and then uploaded.  ``num_classes`` 0: no class_cond (the labels, if any, are ignored).  Otherwise every label was checked
        against ``num_classes`` (at construction, or here for another value) and sample b's is replaced by ``num_classes`` with probability
        ``cond_dropout_rate`` under ``key`` (``class_dropout``)."""
        idx = torch.as_tensor(indices, dtype=torch.int64)
        if idx.is_cuda or idx.dim() != 1 or idx.numel() == 0:
            raise ValueError(f"DeviceImageDataset.batch: indices are a non-empty CPU int64 vector or list (got {idx.device} {tuple(idx.shape)})")
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= self.n:
            raise IndexError(f"DeviceImageDataset.batch: indices span {lo} .. {hi}, outside [0, {self.n})")
        idx = idx.to(self.images.device)
        if not num_classes:
            return batch_u8(self.images, idx)
        if self.labels is None:
            raise ValueError("DeviceImageDataset.batch: num_classes > 0 but the dataset carries no labels")
        if self.max_label >= num_classes:
            raise ValueError(f"DeviceImageDataset.batch: the dataset's labels reach {self.max_label}, outside [0, {num_classes})")
        return batch_u8(self.images, idx, self.labels, key, cond_dropout_rate, num_classes)


# ---- readers of the files torchvision leaves on disk ------------------------------------------------------------------------------------------

def _missing(path, what):
    return FileNotFoundError(f"{what}: expected {path}; nothing is downloaded here, the data must already be there")


def read_cifar10(location):
    """(uint8 [50000, 3, 32, 32], int64 [50000]) from ``location``/cifar-10-batches-py/data_batch_1 .. 5: pickles of a dict whose
    ``data`` is uint8 [n, 3072], each row the R, G and B planes of one image in turn, and whose ``labels`` is a list of n ints."""
    import numpy as np
    images, labels = [], []
    for i in range(1, 6):
        path = Path(location) / "cifar-10-batches-py" / f"data_batch_{i}"
        if not path.is_file():
            raise _missing(path, "read_cifar10")
        with open(path, "rb") as f:
            entry = pickle.load(f, encoding="latin1")
        data = np.asarray(entry["data"], dtype=np.uint8)
        if data.ndim != 2 or data.shape[1] != 3072 or len(entry["labels"]) != data.shape[0]:
            raise ValueError(f"read_cifar10: {path}: data {data.shape}, {len(entry['labels'])} labels; expected [n, 3072] and n labels")
        images.append(torch.from_numpy(data.reshape(-1, 3, 32, 32).copy()))
        labels.append(torch.tensor(list(entry["labels"]), dtype=torch.int64))
    return torch.cat(images), torch.cat(labels)


def _read_idx(path, magic, n_dims, what):
    """The payload of an idx file of unsigned bytes: big-endian magic 0x0000 08 <dims>, then one big-endian uint32 per dimension."""
    if path.is_file():
        raw = path.read_bytes()
    elif Path(str(path) + ".gz").is_file():
        with gzip.open(str(path) + ".gz", "rb") as f:
            raw = f.read()
    else:
        raise _missing(f"{path} (or {path.name}.gz next to it)", what)
    head = 4 + 4 * n_dims
    if len(raw) < head or struct.unpack(">I", raw[:4])[0] != magic:
        raise ValueError(f"{what}: {path}: not an idx file with magic {magic:#010x}")
    dims = struct.unpack(">" + "I" * n_dims, raw[4:head])
    count = 1
    for d in dims:
        count *= d
    if len(raw) - head != count:
        raise ValueError(f"{what}: {path}: header says {dims}, payload holds {len(raw) - head} bytes")
    return torch.frombuffer(bytearray(raw[head:]), dtype=torch.uint8).reshape(dims)


def read_mnist(location):
    """(uint8 [60000, 1, 28, 28], int64 [60000]) from ``location``/MNIST/raw/train-images-idx3-ubyte and train-labels-idx1-ubyte (or the
    ``.gz`` next to either)."""
    raw = Path(location) / "MNIST" / "raw"
    images = _read_idx(raw / "train-images-idx3-ubyte", 0x00000803, 3, "read_mnist")
    labels = _read_idx(raw / "train-labels-idx1-ubyte", 0x00000801, 1, "read_mnist")
    if images.shape[0] != labels.shape[0]:
        raise ValueError(f"read_mnist: {images.shape[0]} images, {labels.shape[0]} labels")
    return images.unsqueeze(1).contiguous(), labels.to(torch.int64)


# ---- the DataLoader types -----------------------------------------------------------------------------------------------------------------------

class FolderOfImagesWithClasses(torch.utils.data.Dataset):
    """One class per immediate subdirectory of ``root`` (the reference's ``imagefolder-class``: torchvision's ImageFolder, without
    torchvision).  ``classes`` is the sorted list of subdirectory names, ``class_to_idx`` maps each to its index; the samples are ordered by
    class, then by sorted path (every depth below the class directory).  Items are ``(image, label)``; without a ``transform`` the image is
    the RGB PIL image.  A class directory without an image is an error."""

    IMG_EXTENSIONS = FolderOfImages.IMG_EXTENSIONS

    def __init__(self, root, transform=None):
        super().__init__()
        self.root = Path(root)
        self.transform = (lambda image: image) if transform is None else transform
        self.classes = sorted(entry.name for entry in os.scandir(self.root) if entry.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"FolderOfImagesWithClasses: no class directory in {self.root}")
        self.class_to_idx = {name: i for i, name in enumerate(self.classes)}
        self.samples = []
        for name in self.classes:
            paths = sorted(path for path in (self.root / name).rglob('*') if path.is_file() and path.suffix.lower() in self.IMG_EXTENSIONS)
            if not paths:
                raise FileNotFoundError(f"FolderOfImagesWithClasses: no image in the class directory {self.root / name} "
                                        f"(extensions: {', '.join(sorted(self.IMG_EXTENSIONS))})")
            self.samples += [(path, self.class_to_idx[name]) for path in paths]

    def __repr__(self):
        return f'FolderOfImagesWithClasses(root="{self.root}", classes: {len(self.classes)}, len: {len(self)})'

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, key):
        from PIL import Image
        path, label = self.samples[key]
        with open(path, 'rb') as f:
            image = Image.open(f).convert('RGB')
        return self.transform(image), label


def load_custom(config_path, dataset_config, transform):
    """The reference's ``custom`` dataset type (train.py:216-223): ``dataset.location`` names a Python file relative to the config file;
    its ``get_dataset`` (or the function ``dataset.get_dataset`` names) is called with ``dataset.config`` and ``transform=``."""
    location = (Path(config_path).parent / dataset_config['location']).resolve()
    if not location.is_file():
        raise FileNotFoundError(f"load_custom: the dataset module {location} does not exist")
    spec = importlib.util.spec_from_file_location('custom_dataset', location)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    get_dataset = getattr(module, dataset_config.get('get_dataset', 'get_dataset'))
    return get_dataset(dataset_config.get('config', {}), transform=transform)

"""Small helpers shared by the sampling path and the training loop (k_diffusion/utils.py equivalents; the EMA update and the sigma
densities run on the HIP kernels of csrc/optim_f32.hip)."""
import json
import math
import struct
import threading
from contextlib import contextmanager
from pathlib import Path

import torch


def append_dims(x, target_dims):
    """Trailing singleton dims until ``x`` has ``target_dims`` dims (utils.py:43-48)."""
    extra = target_dims - x.ndim
    if extra < 0:
        raise ValueError(f"input has {x.ndim} dims but target_dims is {target_dims}, which is less")
    return x.reshape(x.shape + (1,) * extra)


def n_params(module):
    return sum(p.numel() for p in module.parameters())


def to_pil_image(x):
    """[-1, 1] tensor -> PIL image (utils.py:27-34).  The clamp / rescale / 8-bit conversion runs in the
    HIP ``kd_to_uint8`` kernel when ``x`` lives on the GPU (truncating like torchvision's to_pil_image)."""
    from PIL import Image
    if x.ndim == 4:
        assert x.shape[0] == 1
        x = x[0]
    if x.dtype == torch.uint8:                          # already converted on the device (sample.py --gather-uint8)
        u8 = x.cpu()
    elif x.is_cuda:
        from . import ops
        u8 = ops.to_uint8(x.to(torch.float32).contiguous()).cpu()
    else:
        u8 = (((x.float().clamp(-1, 1) + 1) / 2) * 255).to(torch.uint8)
    arr = u8.numpy()
    if arr.shape[0] == 1:
        return Image.fromarray(arr[0], mode="L")
    return Image.fromarray(arr.transpose(1, 2, 0), mode="RGB" if arr.shape[0] == 3 else None)


@contextmanager
def _mode(model, training):
    previous = [m.training for m in model.modules()]
    try:
        yield model.train(training)
    finally:
        for m, was in zip(model.modules(), previous):
            m.training = was


def train_mode(model, mode=True):
    """Context manager / decorator that puts ``model`` in train (or eval) mode and restores it."""
    return _mode(model, mode)


def eval_mode(model):
    return _mode(model, False)


def get_safetensors_metadata(path):
    """The ``__metadata__`` dict of a safetensors file, read from its JSON header only."""
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(n)).get("__metadata__", {})


# ------------------------------------------------------------------------------------------------------------------ training (utils.py:88-426)

def ema_update(model, averaged_model, decay):
    """Incorporates updated model parameters into an exponential moving averaged version of a model; call it after each optimizer step
    (utils.py:88-104).  One kd_mt_lerp_f32 launch over all parameters, then the buffer copies.  ``optim.AdamW.step(ema_decay=...)`` does
    the same inside the optimizer's own pass."""
    from . import optim
    optim.ema_update(model, averaged_model, decay)


def ema_update_dict(values, updates, decay):
    """EMA of a dict of host scalars (utils.py:451-458)."""
    for k, v in updates.items():
        if k not in values:
            values[k] = v
        else:
            values[k] *= decay
            values[k] += (1 - decay) * v
    return values


class EMAWarmup:
    """EMA decay on an inverse-decay warmup schedule (utils.py:107-152): ``1 - (1 + epoch / inv_gamma) ** -power`` clamped to
    [min_value, max_value], with epoch = max(0, last_epoch - start_at)."""

    def __init__(self, inv_gamma=1., power=1., min_value=0., max_value=1., start_at=0, last_epoch=0):
        self.inv_gamma = inv_gamma
        self.power = power
        self.min_value = min_value
        self.max_value = max_value
        self.start_at = start_at
        self.last_epoch = last_epoch

    def state_dict(self):
        return dict(self.__dict__.items())

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)

    def get_value(self):
        epoch = max(0, self.last_epoch - self.start_at)
        value = 1 - (1 + epoch / self.inv_gamma) ** -self.power
        return 0. if epoch < 0 else min(self.max_value, max(self.min_value, value))

    def step(self):
        self.last_epoch += 1


def _check_warmup(warmup):
    if not 0. <= warmup < 1:
        raise ValueError('Invalid value for warmup')
    return warmup


class _ClosedFormLR(torch.optim.lr_scheduler.LRScheduler):
    """A scheduler given by ``_get_closed_form_lr`` alone.  ``verbose`` is accepted and ignored (torch >= 2.7 dropped it from
    LRScheduler.__init__)."""

    def get_lr(self):
        return self._get_closed_form_lr()


class InverseLR(_ClosedFormLR):
    """Inverse decay learning rate schedule with an optional exponential warmup (utils.py:155-193): ``inv_gamma`` steps take the rate to
    (1 / 2) ** power of its start; ``warmup`` in [0, 1), 0 disables; ``min_lr`` floors the decayed rate."""

    def __init__(self, optimizer, inv_gamma=1., power=1., warmup=0., min_lr=0., last_epoch=-1, verbose=False):
        self.inv_gamma = inv_gamma
        self.power = power
        self.warmup = _check_warmup(warmup)
        self.min_lr = min_lr
        super().__init__(optimizer, last_epoch)

    def _get_closed_form_lr(self):
        warmup = 1 - self.warmup ** (self.last_epoch + 1)
        lr_mult = (1 + self.last_epoch / self.inv_gamma) ** -self.power
        return [warmup * max(self.min_lr, base_lr * lr_mult) for base_lr in self.base_lrs]


class ExponentialLR(_ClosedFormLR):
    """Exponential learning rate schedule with an optional exponential warmup (utils.py:196-234): the rate falls by ``decay`` every
    ``num_steps`` steps, continuously."""

    def __init__(self, optimizer, num_steps, decay=0.5, warmup=0., min_lr=0., last_epoch=-1, verbose=False):
        self.num_steps = num_steps
        self.decay = decay
        self.warmup = _check_warmup(warmup)
        self.min_lr = min_lr
        super().__init__(optimizer, last_epoch)

    def _get_closed_form_lr(self):
        warmup = 1 - self.warmup ** (self.last_epoch + 1)
        lr_mult = (self.decay ** (1 / self.num_steps)) ** self.last_epoch
        return [warmup * max(self.min_lr, base_lr * lr_mult) for base_lr in self.base_lrs]


class ConstantLRWithWarmup(_ClosedFormLR):
    """Constant learning rate with an optional exponential warmup (utils.py:237-264)."""

    def __init__(self, optimizer, warmup=0., last_epoch=-1, verbose=False):
        self.warmup = _check_warmup(warmup)
        super().__init__(optimizer, last_epoch)

    def _get_closed_form_lr(self):
        warmup = 1 - self.warmup ** (self.last_epoch + 1)
        return [warmup * base_lr for base_lr in self.base_lrs]


def stratified_uniform(shape, group=0, groups=1, dtype=None, device=None):
    """Stratified uniform draws (utils.py:267-276): sample i of the last dimension lies in stratum ``group + i * groups`` of
    ``shape[-1] * groups``."""
    if groups <= 0:
        raise ValueError(f"groups must be positive, got {groups}")
    if group < 0 or group >= groups:
        raise ValueError(f"group must be in [0, {groups})")
    n = shape[-1] * groups
    offsets = torch.arange(group, n, groups, dtype=dtype, device=device)
    u = torch.rand(shape, dtype=dtype, device=device)
    return (offsets + u) / n


stratified_settings = threading.local()


@contextmanager
def enable_stratified(group=0, groups=1, disable=False):
    """Context manager that makes the ``rand_*`` densities draw stratified (utils.py:282-293)."""
    try:
        stratified_settings.disable = disable
        stratified_settings.group = group
        stratified_settings.groups = groups
        yield
    finally:
        del stratified_settings.disable
        del stratified_settings.group
        del stratified_settings.groups


def _strata():
    """(group, groups) of the enclosing enable_stratified, or (0, 0) outside one / when disabled."""
    if not hasattr(stratified_settings, 'disable') or stratified_settings.disable:
        return 0, 0
    group, groups = stratified_settings.group, stratified_settings.groups
    if groups <= 0:
        raise ValueError(f"groups must be positive, got {groups}")
    if group < 0 or group >= groups:
        raise ValueError(f"group must be in [0, {groups})")
    return group, groups


def stratified_with_settings(shape, dtype=None, device=None):
    """Uniform draws, stratified by the enclosing ``enable_stratified`` (utils.py:313-320)."""
    group, groups = _strata()
    if not groups:
        return torch.rand(shape, dtype=dtype, device=device)
    return stratified_uniform(shape, group, groups, dtype=dtype, device=device)


def _density(kind, shape, params, device, dtype, stratified=True, normal=False, wide=False):
    """The draw (torch.rand / torch.randn on the device, as the sampler's start noise) and its transform (kd_sigma_density_f32, with the
    stratification of the enclosing enable_stratified folded in).  ``wide``: fp64 uniforms whatever ``dtype`` (the log-logistic)."""
    from . import _native as nat, ops
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"sigma densities: the HIP path needs a ROCm device (got {device}); there is no CPU fallback")
    draw = torch.float64 if wide or dtype == torch.float64 else torch.float32
    group, groups = _strata() if stratified else (0, 0)
    u = torch.rand(shape, device=device, dtype=draw)
    n = torch.randn(shape, device=device, dtype=draw) if normal else None
    out = ops.sigma_density(getattr(nat, "DENSITY_" + kind), u, params, normal=n, group=group, groups=groups, dtype=dtype)
    return out if out.dtype == dtype else out.to(dtype)


def rand_log_normal(shape, loc=0., scale=1., device='cpu', dtype=torch.float32):
    """Draws samples from a lognormal distribution (utils.py:323-326)."""
    return _density("LOGNORMAL", shape, [loc, scale], device, dtype)


def _sigmoid(x):
    return 1 / (1 + math.exp(-x)) if x >= 0 else math.exp(x) / (1 + math.exp(x))


def _log(x):
    return -math.inf if x == 0 else math.log(x)


def log_logistic_params(loc, scale, min_value, max_value):
    """The truncated log-logistic's kernel constants: loc, scale and the CDF at both bounds, in fp64 (utils.py:331-334)."""
    return [loc, scale, _sigmoid((_log(min_value) - loc) / scale), _sigmoid((_log(max_value) - loc) / scale)]


def rand_log_logistic(shape, loc=0., scale=1., min_value=0., max_value=float('inf'), device='cpu', dtype=torch.float32):
    """Draws samples from an optionally truncated log-logistic distribution (utils.py:329-336; fp64 uniforms and arithmetic)."""
    return _density("LOGLOGISTIC", shape, log_logistic_params(loc, scale, min_value, max_value), device, dtype, wide=True)


def rand_log_uniform(shape, min_value, max_value, device='cpu', dtype=torch.float32):
    """Draws samples from a log-uniform distribution (utils.py:339-343)."""
    return _density("LOGUNIFORM", shape, [math.log(min_value), math.log(max_value)], device, dtype)


def v_diffusion_params(sigma_data, min_value, max_value):
    return [sigma_data, math.atan(min_value / sigma_data) * 2 / math.pi, math.atan(max_value / sigma_data) * 2 / math.pi]


def rand_v_diffusion(shape, sigma_data=1., min_value=0., max_value=float('inf'), device='cpu', dtype=torch.float32):
    """Draws samples from a truncated v-diffusion training timestep distribution (utils.py:346-351)."""
    return _density("V_DIFFUSION", shape, v_diffusion_params(sigma_data, min_value, max_value), device, dtype)


def cosine_interpolated_params(image_d, noise_d_low, noise_d_high, sigma_data, min_value, max_value):
    """t_min, t_max and shift of the cosine log-SNR schedule shifted to noise_d_low, the same of noise_d_high, sigma_data (utils.py:357-372)."""
    logsnr_min = -2 * math.log(min_value / sigma_data)
    logsnr_max = -2 * math.log(max_value / sigma_data)
    out = []
    for noise_d in (noise_d_low, noise_d_high):
        shift = 2 * math.log(noise_d / image_d)
        out += [math.atan(math.exp(-0.5 * (logsnr_max - shift))), math.atan(math.exp(-0.5 * (logsnr_min - shift))), shift]
    return out + [sigma_data]


def rand_cosine_interpolated(shape, image_d, noise_d_low, noise_d_high, sigma_data=1., min_value=1e-3, max_value=1e3, device='cpu',
                             dtype=torch.float32):
    """Draws samples from an interpolated cosine timestep distribution (from simple diffusion; utils.py:354-375)."""
    return _density("COSINE_INTERPOLATED", shape, cosine_interpolated_params(image_d, noise_d_low, noise_d_high, sigma_data, min_value, max_value),
                    device, dtype)


def rand_split_log_normal(shape, loc, scale_1, scale_2, device='cpu', dtype=torch.float32):
    """Draws samples from a split lognormal distribution (utils.py:378-385; never stratified, as in the reference)."""
    return _density("SPLIT_LOGNORMAL", shape, [loc, scale_1, scale_2, scale_1 / (scale_1 + scale_2)], device, dtype, stratified=False, normal=True)


class FolderOfImages(torch.utils.data.Dataset):
    """Recursively finds all images in a directory; no classes / targets (utils.py:388-411).  Items are 1-tuples ``(image,)``; without a
    ``transform`` the image is the RGB PIL image."""

    IMG_EXTENSIONS = {'.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp'}

    def __init__(self, root, transform=None):
        super().__init__()
        self.root = Path(root)
        self.transform = (lambda image: image) if transform is None else transform
        self.paths = sorted(path for path in self.root.rglob('*') if path.suffix.lower() in self.IMG_EXTENSIONS)

    def __repr__(self):
        return f'FolderOfImages(root="{self.root}", len: {len(self)})'

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, key):
        from PIL import Image
        with open(self.paths[key], 'rb') as f:
            image = Image.open(f).convert('RGB')
        return self.transform(image),


def resize_center_crop(image, size):
    """PIL only (torchvision is not a dependency): the shorter side to ``size`` with LANCZOS, then the centre ``size`` x ``size`` crop."""
    from PIL import Image
    w, h = image.size
    if w <= h:
        nw, nh = size, max(size, int(size * h / w))
    else:
        nw, nh = max(size, int(size * w / h)), size
    if (nw, nh) != (w, h):
        image = image.resize((nw, nh), Image.LANCZOS)
    left, top = (nw - size) // 2, (nh - size) // 2
    return image.crop((left, top, left + size, top + size))


def from_pil_image(image):
    """PIL image -> [C, H, W] fp32 tensor in [-1, 1] (utils.py:19-24)."""
    import numpy as np
    arr = np.asarray(image, dtype=np.uint8)
    if arr.ndim == 2:
        arr = arr[..., None]
    return torch.from_numpy(arr.copy()).permute(2, 0, 1).to(torch.float32) / 255 * 2 - 1


class CSVLogger:
    """Appends rows to a CSV file, writing the header when the file is new (utils.py:414-425)."""

    def __init__(self, filename, columns):
        self.filename = Path(filename)
        self.columns = columns
        if self.filename.exists():
            self.file = open(self.filename, 'a')
        else:
            self.file = open(self.filename, 'w')
            self.write(*self.columns)

    def write(self, *args):
        print(*args, sep=',', file=self.file, flush=True)

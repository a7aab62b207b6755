"""Karras et al. (2022) augmentation on the device: the reference's ``k_diffusion/augmentation.py`` (``KarrasAugmentationPipeline``,
``KarrasAugmentWrapper``) over this project's HIP kernels (csrc/augment_f32.hip; arithmetic and counter contract: include/kdiff_hip.h).

The reference augments one PIL image at a time on CPU data-loader workers and warps it with scikit-image.  Here the pipeline is a batched
device op on the uploaded batch: ``pipeline.batch(images)`` draws eight parameters per sample from this project's counter-based generator
-- NOT the torch RNG stream of the reference -- and warps every sample in one launch.  There is no CPU path.

``augment_draw`` / ``augment_warp`` are the tensor-level wrappers over the C ABI (the module's counterpart of ``ops``).
"""
import torch
from torch import nn

from . import _native as nat
from .ops import _chk, _p, _stream


def augment_draw(key, batch, a_prob, out=None):
    """raw [batch, 8] = (a0 .. a7) per sample from ``key`` (a one-element int64 device tensor): ``kd_augment_draw_f32``, the reference's
    draws (augmentation.py:44-70) on the counter contract of include/kdiff_hip.h.  The same key gives the same bits."""
    if _chk(key, "key", torch.int64).numel() != 1:
        raise ValueError(f"augment_draw: the key is one int64 (got {key.numel()} elements)")
    batch = int(batch)
    out = torch.empty(batch, 8, device=key.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "out").shape) != (batch, 8):
        raise ValueError(f"augment_draw: out shape {tuple(out.shape)} != {(batch, 8)}")
    nat.check(nat.lib().kd_augment_draw_f32(_p(key), batch, float(a_prob), _p(out), _stream()), "kd_augment_draw_f32")
    return out


def augment_warp(x, raw, a_scale=2 ** 0.2, a_aniso=2 ** 0.2, a_trans=1 / 8, out=None, with_mat=False):
    """(y, cond) -- or (y, cond, mat) with ``with_mat`` -- for x [B, C, H, W] and raw [B, 8]: ``kd_augment_warp_f32``.  y is x warped by the
    inverse of the reference's matrix (bicubic, reflect), cond [B, 9] its conditioning vector (augmentation.py:75), mat [B, 6] the top two
    rows of the inverse map.  ``out`` must not overlap x; H, W >= 2."""
    if _chk(x, "x").dim() != 4:
        raise ValueError(f"augment_warp: x is [B, C, H, W] (got {tuple(x.shape)})")
    B, C, H, W = x.shape
    if tuple(_chk(raw, "raw").shape) != (B, 8):
        raise ValueError(f"augment_warp: raw shape {tuple(raw.shape)} != {(B, 8)}")
    out = torch.empty_like(x) if out is None else out
    if _chk(out, "out").shape != x.shape:
        raise ValueError(f"augment_warp: out shape {tuple(out.shape)} != {tuple(x.shape)}")
    cond = torch.empty(B, 9, device=x.device, dtype=torch.float32)
    mat = torch.empty(B, 6, device=x.device, dtype=torch.float32) if with_mat else None
    nat.check(nat.lib().kd_augment_warp_f32(_p(x), _p(raw), float(a_scale), float(a_aniso), float(a_trans), _p(out), _p(cond), _p(mat),
                                            B, C, H, W, _stream()), "kd_augment_warp_f32")
    return (out, cond, mat) if with_mat else (out, cond)


class KarrasAugmentationPipeline:
    """The reference's pipeline (augmentation.py:32-89) with its constructor and attributes.  ``batch`` is the device form; ``__call__`` keeps
    the reference's per-image signature on top of it."""

    def __init__(self, a_prob=0.12, a_scale=2**0.2, a_aniso=2**0.2, a_trans=1/8, disable_all=False):
        self.a_prob = a_prob
        self.a_scale = a_scale
        self.a_aniso = a_aniso
        self.a_trans = a_trans
        self.disable_all = disable_all

    def batch(self, images, generator=None, raw=None):
        """images [B, C, H, W] fp32 on the ROCm device, in [-1, 1] -> (image, image_orig, cond): the augmented batch, ``images`` itself, and
        cond [B, 9].  Each call draws one int64 key from ``generator`` (a torch.Generator on the images' device; None: that device's default
        generator, so torch.manual_seed governs it -- as ``enable_dropout`` draws its key) and the parameters from the key on the device; the
        reference's torch draws are not reproduced.  ``raw`` [B, 8] = (a0 .. a7) bypasses the draw (no key is consumed).  With
        ``disable_all`` the image is the input itself and cond is zero, as in the reference."""
        if _chk(images, "images").dim() != 4:
            raise ValueError(f"KarrasAugmentationPipeline.batch: images are [B, C, H, W] (got {tuple(images.shape)})")
        if generator is not None and not isinstance(generator, torch.Generator):
            raise TypeError(f"KarrasAugmentationPipeline.batch: generator must be a torch.Generator or None (got {type(generator)})")
        B = images.shape[0]
        if self.disable_all:
            return images, images, images.new_zeros([B, 9])
        if raw is None:
            key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=images.device, generator=generator)
            raw = augment_draw(key, B, self.a_prob)
        image, cond = augment_warp(images, raw, self.a_scale, self.a_aniso, self.a_trans)
        return image, images, cond

    def __call__(self, image, generator=None):
        """The reference's per-image form: a PIL image -> (image, image_orig, cond) as [C, H, W], [C, H, W] and [9] tensors on the device
        (``batch`` with B = 1)."""
        from .utils import from_pil_image
        x = from_pil_image(image).unsqueeze(0).contiguous().to(torch.device("cuda"))
        image, image_orig, cond = self.batch(x, generator=generator)
        return image[0], image_orig[0], cond[0]


class KarrasAugmentWrapper(nn.Module):
    """augmentation.py:92-113: feeds ``aug_cond`` (zeros [B, 9] when none is given) to an inner model that takes ``mapping_cond`` only, in
    front of the caller's ``mapping_cond``.  (This project's ImageTransformerDenoiserModelV2 takes ``aug_cond`` itself and needs no wrapper.)"""

    def __init__(self, model):
        super().__init__()
        self.inner_model = model

    def forward(self, input, sigma, aug_cond=None, mapping_cond=None, **kwargs):
        cond = input.new_zeros([input.shape[0], 9]) if aug_cond is None else aug_cond
        if mapping_cond is not None:
            cond = torch.cat([cond, mapping_cond], dim=1)
        return self.inner_model(input, sigma, mapping_cond=cond, **kwargs)

    # what train.py asks of the model it wraps
    def param_groups(self, *args, **kwargs):
        return self.inner_model.param_groups(*args, **kwargs)

    def set_skip_stages(self, skip_stages):
        return self.inner_model.set_skip_stages(skip_stages)

    def set_patch_size(self, patch_size):
        return self.inner_model.set_patch_size(patch_size)

    def enable_dropout(self, generator=None):
        """The inner model's ``enable_dropout`` (opt-in dropout of the training loss); returns this wrapper."""
        self.inner_model.enable_dropout(generator)
        return self

    def set_wgrad_arithmetic(self, arithmetic=None):
        """The inner model's ``set_wgrad_arithmetic`` (opt-in bf16 weight gradients of the training loss); returns this wrapper."""
        self.inner_model.set_wgrad_arithmetic(arithmetic)
        return self

    def set_conv_arithmetic(self, arithmetic=None):
        """The inner model's ``set_conv_arithmetic`` (opt-in bf16 convolutions of the sampling forward); returns this wrapper."""
        self.inner_model.set_conv_arithmetic(arithmetic)
        return self

    def _dropout_rates(self):
        return self.inner_model._dropout_rates()

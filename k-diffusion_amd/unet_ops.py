"""Tensor-level wrappers over the C ABI of the image_v1 U-Net kernels (csrc/conv_x3.hip, csrc/unet_f32.hip; contracts: include/kdiff_hip.h)
and of their reverse rules (csrc/unet_vjp_f32.hip; contracts: include/kdiff_unet_grad.h) and parameter-gradient rules (csrc/conv_wgrad_x3.hip,
csrc/unet_train_f32.hip; contracts: include/kdiff_unet_train.h) and dropout kernels (csrc/unet_drop_f32.hip and one entry point each of
csrc/conv_x3.hip and csrc/vjp_f32.hip; contracts: include/kdiff_unet_drop.h) and of the bf16 forms of the convolution and of its weight gradient
(csrc/conv_bf16.hip, csrc/conv_wgrad_bf16.hip; contracts: include/kdiff_unet_bf16.h, include/kdiff_unet_mixed.h) -- the module's counterpart of
``ops``, as ``augmentation`` and ``data`` have theirs.

Activations are fp32 NHWC, token-major: a 2-D tensor ``[B * H * W, C]`` whose row stride may exceed C (a column range of a wider buffer:
``buf[:, :C]`` and ``buf[:, C:]`` are the two halves of a skip concatenation, written in place by their producers).  Column 0 of such a view
must stay 16-byte aligned.  ROCm tensors only; there is no CPU path.
"""
import math

import torch

from . import _native as nat
from . import ops
from . import weights
from .ops import _chk, _p, _stream


def _rows(t, name, chan=None):
    """A token-major activation: 2-D fp32 on the device, unit column stride; returns its row stride."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a tensor on a ROCm device (got {t.device}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1 or (chan is not None and t.shape[1] != chan):
        raise ValueError(f"{name}: expected [tokens, {chan or 'C'}] with unit column stride (got {tuple(t.shape)}, strides {t.stride()})")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    if ld < t.shape[1]:
        raise ValueError(f"{name}: row stride {ld} shorter than the row")
    return ld


def _tokens(x, B, H, W, name):
    if x.shape[0] != B * H * W:
        raise ValueError(f"{name}: {x.shape[0]} rows for batch {B} x {H} x {W}")


_packed = weights.WeakCache()


def pack_conv(weight, cache=True):
    """Packed split-bf16 image of a conv weight [C_out, C_in, ks, ks] (``kd_pack_conv_x3``), cached per tensor object (``weights.WeakCache``)."""
    def build():
        if _chk(weight, "weight").dim() != 4 or weight.shape[2] != weight.shape[3]:
            raise ValueError(f"pack_conv: weight is [C_out, C_in, ks, ks] (got {tuple(weight.shape)})")
        c_out, c_in, ks, _ = weight.shape
        img = torch.empty(4 * ks * ks * c_out * c_in, device=weight.device, dtype=torch.uint8)
        nat.check(nat.lib().kd_pack_conv_x3(_p(weight), _p(img), c_out, c_in, ks, _stream()), "kd_pack_conv_x3")
        return img
    return _packed.get(weight, None, None, build, cache=cache)


def conv2d(x, weight, B, H, W, bias=None, residual=None, out=None, packed=None, bias_batch=None, chan_scale=None, bf16=False):
    """conv2d(x, weight, padding=ks // 2) + bias + residual on tokens x [B*H*W, C_in] -> [B*H*W, C_out] (``kd_conv2d_x3``), ks 1 or 3.
    ``out`` must not overlap x.  With ``bias_batch`` only the samples b < bias_batch get the bias (``kd_conv2d_x3_stacked``: a dual pass's
    batch is [primal | tangent], and the tangent of conv(x) + bias has no bias).  With ``chan_scale`` [B, C_out] (a site's column range of
    ``chan_mask``'s table) the channel dropout of the training loss rides in the epilogue: (conv + bias) * chan_scale[b] + residual
    (``kd_conv2d_x3_drop``).  ``bf16``: activations and weights rounded once to bf16, one bf16 MFMA per product with fp32 accumulation
    (``kd_conv2d_bf16``, include/kdiff_unet_bf16.h; the same packed image) -- the same contract otherwise, for the sampling forward alone: not
    together with ``bias_batch`` or ``chan_scale``."""
    if bf16 and (bias_batch is not None or chan_scale is not None):
        raise ValueError(f"conv2d: bf16 excludes {'bias_batch' if bias_batch is not None else 'chan_scale'}: the dual pass (bias_batch) and the "
                         "training loss (chan_scale) keep the fp32-grade arithmetic")
    c_out, c_in, ks, _ = weight.shape
    ldx = _rows(x, "x", c_in)
    _tokens(x, B, H, W, "conv2d")
    out = torch.empty(x.shape[0], c_out, device=x.device, dtype=torch.float32) if out is None else out
    ldy = _rows(out, "out", c_out)
    ldr = _rows(residual, "residual", c_out) if residual is not None else 0
    if out.shape[0] != x.shape[0] or (residual is not None and residual.shape[0] != x.shape[0]):
        raise ValueError("conv2d: out and residual have the rows of x")
    packed = pack_conv(weight) if packed is None else packed
    args = (_p(x), ldx, _p(packed), _p(None if bias is None else _chk(bias, "bias")), _p(residual), ldr, _p(out), ldy, B, H, W, c_in, c_out, ks)
    if bf16:
        nat.check(nat.lib().kd_conv2d_bf16(*args, _stream()), "kd_conv2d_bf16")
    elif chan_scale is not None:
        if bias_batch is not None:
            raise ValueError("conv2d: chan_scale (the training loss's dropout) and bias_batch (the dual pass) exclude each other")
        cs = _rows(chan_scale, "chan_scale", c_out)
        if chan_scale.shape[0] != B:
            raise ValueError(f"conv2d: chan_scale {tuple(chan_scale.shape)} != {(B, c_out)}")
        nat.check(nat.lib().kd_conv2d_x3_drop(*args[:6], _p(chan_scale), cs, *args[6:], _stream()), "kd_conv2d_x3_drop")
    elif bias_batch is None:
        nat.check(nat.lib().kd_conv2d_x3(*args, _stream()), "kd_conv2d_x3")
    else:
        nat.check(nat.lib().kd_conv2d_x3_stacked(*args, int(bias_batch), _stream()), "kd_conv2d_x3_stacked")
    return out


def groupnorm_stats(x, B, groups, eps=1e-5, out=None):
    """stats [B, groups, 4] = (mean_hi, mean_lo, rstd, 0) of tokens x [B*HW, C] (``kd_groupnorm_stats_f32``)."""
    ldx = _rows(x, "x")
    hw, chan = x.shape[0] // B, x.shape[1]
    out = torch.empty(B, groups, 4, device=x.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "stats").shape) != (B, groups, 4) or hw * B != x.shape[0]:
        raise ValueError(f"groupnorm_stats: stats {tuple(out.shape)} / rows {x.shape[0]} for batch {B}, {groups} groups")
    nat.check(nat.lib().kd_groupnorm_stats_f32(_p(x), ldx, _p(out), B, hw, chan, groups, float(eps), _stream()), "kd_groupnorm_stats_f32")
    return out


def adagn_apply(x, stats, wb, gelu=False, out=None):
    """(x - mean) rstd (1 + w) + b per sample, then optionally exact GELU (``kd_adagn_apply_f32``); wb [B, >= 2 C] with unit column stride holds
    (w, b) of each sample in its first 2 C columns."""
    ldx = _rows(x, "x")
    B, groups = stats.shape[:2]
    hw, chan = x.shape[0] // B, x.shape[1]
    wbs = _rows(wb, "wb")
    if wb.shape[0] != B or wb.shape[1] != 2 * chan:
        raise ValueError(f"adagn_apply: wb {tuple(wb.shape)} != {(B, 2 * chan)}")
    out = torch.empty(x.shape[0], chan, device=x.device, dtype=torch.float32) if out is None else out
    ldy = _rows(out, "out", chan)
    nat.check(nat.lib().kd_adagn_apply_f32(_p(x), ldx, _p(_chk(stats, "stats")), _p(wb), wbs, _p(out), ldy, B, hw, chan, groups, int(bool(gelu)),
                                           _stream()), "kd_adagn_apply_f32")
    return out


def _dual(x, x_dot, name):
    """Row strides of a primal and its tangent, which has the primal's shape."""
    ldx, ldxd = _rows(x, name), _rows(x_dot, name + "_dot")
    if x_dot.shape != x.shape:
        raise ValueError(f"{name}_dot: tangent shape {tuple(x_dot.shape)} != primal shape {tuple(x.shape)}")
    return ldx, ldxd


def groupnorm_stats_jvp(x, x_dot, B, groups, eps=1e-5, out=None, out_dot=None):
    """(stats, jstats): ``groupnorm_stats(x)`` with the same bits, and jstats [B, groups, 4] = (mean_dot, rstd_dot, 0, 0), the statistics'
    tangents along x_dot (``kd_groupnorm_stats_jvp_f32``)."""
    ldx, ldxd = _dual(x, x_dot, "x")
    hw, chan = x.shape[0] // B, x.shape[1]
    out = torch.empty(B, groups, 4, device=x.device, dtype=torch.float32) if out is None else out
    out_dot = torch.empty(B, groups, 4, device=x.device, dtype=torch.float32) if out_dot is None else out_dot
    if tuple(_chk(out, "stats").shape) != (B, groups, 4) or tuple(_chk(out_dot, "jstats").shape) != (B, groups, 4) or hw * B != x.shape[0]:
        raise ValueError(f"groupnorm_stats_jvp: stats {tuple(out.shape)}, jstats {tuple(out_dot.shape)} / rows {x.shape[0]} for batch {B}, "
                         f"{groups} groups")
    nat.check(nat.lib().kd_groupnorm_stats_jvp_f32(_p(x), ldx, _p(x_dot), ldxd, _p(out), _p(out_dot), B, hw, chan, groups, float(eps), _stream()),
              "kd_groupnorm_stats_jvp_f32")
    return out, out_dot


def adagn_apply_jvp(x, x_dot, stats, jstats, wb, gelu=False, out=None, out_dot=None):
    """(y, y_dot): ``adagn_apply(x, stats, wb, gelu)`` with the same bits, and its tangent along x_dot with the conditioning ``wb`` held fixed
    (``kd_adagn_apply_jvp_f32``).  ``out`` may be x together with ``out_dot`` being x_dot (in place)."""
    ldx, ldxd = _dual(x, x_dot, "x")
    B, groups = stats.shape[:2]
    hw, chan = x.shape[0] // B, x.shape[1]
    wbs = _rows(wb, "wb")
    if wb.shape[0] != B or wb.shape[1] != 2 * chan:
        raise ValueError(f"adagn_apply_jvp: wb {tuple(wb.shape)} != {(B, 2 * chan)}")
    if tuple(_chk(jstats, "jstats").shape) != tuple(_chk(stats, "stats").shape) or hw * B != x.shape[0]:
        raise ValueError(f"adagn_apply_jvp: stats {tuple(stats.shape)}, jstats {tuple(jstats.shape)} / rows {x.shape[0]} for batch {B}")
    out = torch.empty(x.shape[0], chan, device=x.device, dtype=torch.float32) if out is None else out
    out_dot = torch.empty(x.shape[0], chan, device=x.device, dtype=torch.float32) if out_dot is None else out_dot
    ldy, ldyd = _dual(out, out_dot, "out")
    if out.shape != x.shape:
        raise ValueError(f"adagn_apply_jvp: out {tuple(out.shape)} != x {tuple(x.shape)}")
    nat.check(nat.lib().kd_adagn_apply_jvp_f32(_p(x), ldx, _p(x_dot), ldxd, _p(stats), _p(jstats), _p(wb), wbs, _p(out), ldy, _p(out_dot), ldyd, B, hw,
                                               chan, groups, int(bool(gelu)), _stream()), "kd_adagn_apply_jvp_f32")
    return out, out_dot


def _resample(entry, x, B, H, W, out, Ho, Wo):
    ldx = _rows(x, "x")
    _tokens(x, B, H, W, entry)
    chan = x.shape[1]
    out = torch.empty(B * Ho * Wo, chan, device=x.device, dtype=torch.float32) if out is None else out
    ldy = _rows(out, "out", chan)
    if out.shape[0] != B * Ho * Wo:
        raise ValueError(f"{entry}: out has {out.shape[0]} rows, expected {B * Ho * Wo}")
    nat.check(getattr(nat.lib(), entry)(_p(x), ldx, _p(out), ldy, B, H, W, chan, _stream()), entry)
    return out


def down2(x, B, H, W, out=None):
    """Downsample2d('linear', 'reflect') on tokens: [B*H*W, C] -> [B*(H/2)*(W/2), C] (``kd_down2_f32``)."""
    return _resample("kd_down2_f32", x, B, H, W, out, H // 2, W // 2)


def up2(x, B, H, W, out=None):
    """Upsample2d('linear', 'reflect') on tokens: [B*H*W, C] -> [B*2H*2W, C] (``kd_up2_f32``)."""
    return _resample("kd_up2_f32", x, B, H, W, out, 2 * H, 2 * W)


def unet_in(image, weight, bias=None, sigma=None, sigma_data=1.0, out=None):
    """proj_in: NCHW image -> tokens [B*H*W, C] through weight [C, C_img(, 1, 1)]; with ``sigma`` the image is scaled by c_in first."""
    B, c_img, H, W = _chk(image, "image").shape
    chan = weight.shape[0]
    out = torch.empty(B * H * W, chan, device=image.device, dtype=torch.float32) if out is None else out
    ldy = _rows(out, "out", chan)
    nat.check(nat.lib().kd_unet_in_f32(_p(image), _p(_chk(weight, "weight")), _p(None if bias is None else _chk(bias, "bias")),
                                       _p(None if sigma is None else _chk(sigma, "sigma")), float(sigma_data), _p(out), ldy, B, H * W, c_img, chan,
                                       _stream()), "kd_unet_in_f32")
    return out


def unet_out(x, weight, bias, shape, image=None, sigma=None, sigma_data=1.0, out=None):
    """proj_out: tokens [B*H*W, C] -> NCHW ``shape`` through weight [C_img, C(, 1, 1)]; with ``sigma`` (and the input ``image``) the result is
    F c_out + image c_skip."""
    B, c_img, H, W = shape
    ldx = _rows(x, "x", weight.shape[1])
    _tokens(x, B, H, W, "unet_out")
    out = torch.empty(shape, device=x.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "out").shape) != tuple(shape) or weight.shape[0] != c_img:
        raise ValueError(f"unet_out: out {tuple(out.shape)} / weight {tuple(weight.shape)} for {tuple(shape)}")
    nat.check(nat.lib().kd_unet_out_f32(_p(x), ldx, _p(_chk(weight, "weight")), _p(None if bias is None else _chk(bias, "bias")),
                                        _p(None if image is None else _chk(image, "image")), _p(None if sigma is None else _chk(sigma, "sigma")),
                                        float(sigma_data), _p(out), B, H * W, c_img, x.shape[1], _stream()), "kd_unet_out_f32")
    return out


def cond_mlp(x, weight, bias=None, add=None, gelu=False, out=None):
    """act(x W^T + bias + add) for a few rows in exact fp32 (``kd_cond_mlp_f32``): x [R, K], weight [N, K] -> [R, N]."""
    R, K = _chk(x, "x").shape
    N = weight.shape[0]
    if _chk(weight, "weight").shape[1] != K:
        raise ValueError(f"cond_mlp: weight {tuple(weight.shape)} for x {tuple(x.shape)}")
    out = torch.empty(R, N, device=x.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "out").shape) != (R, N) or (add is not None and tuple(_chk(add, "add").shape) != (R, N)):
        raise ValueError(f"cond_mlp: out / add must be {(R, N)}")
    nat.check(nat.lib().kd_cond_mlp_f32(_p(x), _p(weight), _p(None if bias is None else _chk(bias, "bias")), _p(add), _p(out), R, N, K,
                                        int(bool(gelu)), _stream()), "kd_cond_mlp_f32")
    return out


# ---- reverse rules w.r.t. the activations (csrc/unet_vjp_f32.hip): what ``ImageDenoiserModelV1.forward_vjp`` walks back through ----------------------

def pack_conv_dgrad(weight, q_rows=0):
    """Packed image (``pack_conv``'s) of the weight of a convolution's DATA gradient: w'[ci, co, ky, kx] = w[co, ci, ks-1-ky, ks-1-kx], so that
    g_x = conv2d(g_y, w', padding=ks // 2) for a stride-1 convolution with zero padding ks // 2.  ``q_rows``: the first q_rows output channels
    of w carry a folded 1 / 8 (the q rows of a qkv projection, as the forward packs them).  Cached per tensor object and ``q_rows``."""
    def build():
        if _chk(weight, "weight").dim() != 4 or weight.shape[2] != weight.shape[3]:
            raise ValueError(f"pack_conv_dgrad: weight is [C_out, C_in, ks, ks] (got {tuple(weight.shape)})")
        w = weight.detach()
        if q_rows:
            w = w.clone()
            w[:q_rows] *= 0.125
        return pack_conv(w.flip(2, 3).transpose(0, 1).contiguous(), cache=False)
    return _packed.get(weight, ("dgrad", int(q_rows)), None, build)


def conv2d_dgrad(g_y, weight, B, H, W, residual=None, out=None, q_rows=0):
    """g_x [B*H*W, C_in] = the data gradient of ``conv2d(x, weight)`` from g_y [B*H*W, C_out], + residual (``kd_conv2d_x3`` on
    ``pack_conv_dgrad(weight)``; the bias gets no gradient).  ``out`` must not overlap g_y; it may be ``residual`` (g += ...)."""
    c_out, c_in, ks, _ = weight.shape
    ldg = _rows(g_y, "g_y", c_out)
    _tokens(g_y, B, H, W, "conv2d_dgrad")
    out = torch.empty(g_y.shape[0], c_in, device=g_y.device, dtype=torch.float32) if out is None else out
    ldo = _rows(out, "out", c_in)
    ldr = _rows(residual, "residual", c_in) if residual is not None else 0
    if out.shape[0] != g_y.shape[0] or (residual is not None and residual.shape[0] != g_y.shape[0]):
        raise ValueError("conv2d_dgrad: out and residual have the rows of g_y")
    nat.check(nat.lib().kd_conv2d_x3(_p(g_y), ldg, _p(pack_conv_dgrad(weight, q_rows)), None, _p(residual), ldr, _p(out), ldo, B, H, W, c_out, c_in,
                                     ks, _stream()), "kd_conv2d_x3")
    return out


def _adagn_vjp_dims(entry, x, stats, wb, g_y):
    ldx, ldgy = _rows(x, "x"), _rows(g_y, "g_y")
    if g_y.shape != x.shape:
        raise ValueError(f"{entry}: g_y shape {tuple(g_y.shape)} != x shape {tuple(x.shape)}")
    if _chk(stats, "stats").dim() != 3 or stats.shape[2] != 4:
        raise ValueError(f"{entry}: stats is [B, groups, 4] (got {tuple(stats.shape)})")
    B, groups = stats.shape[:2]
    hw, chan = x.shape[0] // B, x.shape[1]
    wbs = _rows(wb, "wb")
    if wb.shape[0] != B or wb.shape[1] != 2 * chan:
        raise ValueError(f"{entry}: wb {tuple(wb.shape)} != {(B, 2 * chan)}")
    if hw * B != x.shape[0]:
        raise ValueError(f"{entry}: {x.shape[0]} rows for batch {B}")
    return ldx, ldgy, wbs, B, groups, hw, chan


def adagn_vjp_stats(x, stats, wb, g_y, gelu=False, out=None):
    """gstats [B, groups, 4] = (mean(g_xh), mean(g_xh xh), 0, 0) per (sample, group): the two means of the reverse of ``adagn_apply(x, stats,
    wb, gelu)`` from the gradient g_y on its output (``kd_adagn_vjp_stats_f32``)."""
    ldx, ldgy, wbs, B, groups, hw, chan = _adagn_vjp_dims("adagn_vjp_stats", x, stats, wb, g_y)
    out = torch.empty(B, groups, 4, device=x.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "gstats").shape) != (B, groups, 4):
        raise ValueError(f"adagn_vjp_stats: gstats {tuple(out.shape)} != {(B, groups, 4)}")
    nat.check(nat.lib().kd_adagn_vjp_stats_f32(_p(x), ldx, _p(stats), _p(wb), wbs, _p(g_y), ldgy, _p(out), B, hw, chan, groups, int(bool(gelu)),
                                               _stream()), "kd_adagn_vjp_stats_f32")
    return out


def adagn_vjp_apply(x, stats, gstats, wb, g_y, g_add=None, gelu=False, out=None):
    """g_x = the gradient of ``adagn_apply(x, stats, wb, gelu)`` w.r.t. x from g_y, the conditioning ``wb`` held fixed, + g_add
    (``kd_adagn_vjp_apply_f32``).  ``out`` may be g_y or g_add (in place), not x."""
    ldx, ldgy, wbs, B, groups, hw, chan = _adagn_vjp_dims("adagn_vjp_apply", x, stats, wb, g_y)
    if tuple(_chk(gstats, "gstats").shape) != tuple(stats.shape):
        raise ValueError(f"adagn_vjp_apply: gstats {tuple(gstats.shape)} != stats {tuple(stats.shape)}")
    ldga = _rows(g_add, "g_add", chan) if g_add is not None else 0
    out = torch.empty(x.shape[0], chan, device=x.device, dtype=torch.float32) if out is None else out
    ldgx = _rows(out, "out", chan)
    if out.shape[0] != x.shape[0] or (g_add is not None and g_add.shape[0] != x.shape[0]):
        raise ValueError("adagn_vjp_apply: out and g_add have the rows of x")
    nat.check(nat.lib().kd_adagn_vjp_apply_f32(_p(x), ldx, _p(stats), _p(gstats), _p(wb), wbs, _p(g_y), ldgy, _p(g_add), ldga, _p(out), ldgx, B, hw,
                                               chan, groups, int(bool(gelu)), _stream()), "kd_adagn_vjp_apply_f32")
    return out


def _resample_vjp(entry, g_y, B, H, W, Ho, Wo, out, accumulate):
    ldgy = _rows(g_y, "g_y")
    _tokens(g_y, B, Ho, Wo, entry)
    chan = g_y.shape[1]
    if out is None:
        if accumulate:
            raise ValueError(f"{entry}: accumulate needs the tensor to add to (out)")
        out = torch.empty(B * H * W, chan, device=g_y.device, dtype=torch.float32)
    ldgx = _rows(out, "out", chan)
    if out.shape[0] != B * H * W:
        raise ValueError(f"{entry}: out has {out.shape[0]} rows, expected {B * H * W}")
    nat.check(getattr(nat.lib(), entry)(_p(g_y), ldgy, _p(out), ldgx, B, H, W, chan, int(bool(accumulate)), _stream()), entry)
    return out


def down2_vjp(g_y, B, H, W, out=None, accumulate=False):
    """The transpose of ``down2`` at input size H x W: g_y [B*(H/2)*(W/2), C] -> g_x [B*H*W, C] (``kd_down2_vjp_f32``); with ``accumulate`` it is
    added to ``out``."""
    return _resample_vjp("kd_down2_vjp_f32", g_y, B, H, W, H // 2, W // 2, out, accumulate)


def up2_vjp(g_y, B, H, W, out=None, accumulate=False):
    """The transpose of ``up2`` at input size H x W: g_y [B*2H*2W, C] -> g_x [B*H*W, C] (``kd_up2_vjp_f32``); with ``accumulate`` it is added
    to ``out``."""
    return _resample_vjp("kd_up2_vjp_f32", g_y, B, H, W, 2 * H, 2 * W, out, accumulate)


# ---- parameter gradients (csrc/conv_wgrad_x3.hip, csrc/unet_train_f32.hip; contracts: include/kdiff_unet_train.h): what the backward of
# ``ImageDenoiserModelV1.loss_forward`` launches beside the reverse rules above ------------------------------------------------------------------------

CONV_WGRAD_BLOCKS = 256     # workgroups kd_conv2d_wgrad_x3 aims at: one per CU; the pixel sum is cut until (co, ci) tiles x chunks reach it


def conv_wgrad_chunks(B, H, W, c_in, c_out):
    """(patches_per_chunk, nchunk) of ``kd_conv2d_wgrad_x3``: how the sum over the B ceil(H / 8) ceil(W / 8) pixel patches is cut into partial
    sums.  A fixed function of the shape, so that the order of the sum is too."""
    patches = B * -(-H // 8) * -(-W // 8)
    tiles = (c_in // 64) * (c_out // 64)
    nchunk = max(1, min(-(-CONV_WGRAD_BLOCKS // max(tiles, 1)), patches))
    per_chunk = -(-patches // nchunk)
    return per_chunk, -(-patches // per_chunk)


def conv2d_wgrad(g, a, B, H, W, ks, out=None, accumulate=False, q_rows=0, chunks=None, bf16=False):
    """dW [C_out, C_in, ks, ks] (+)= the weight gradient of ``conv2d(a, weight)`` (ks 1 or 3, padding ks // 2) from the gradient g
    [B*H*W, C_out] on its output and its input a [B*H*W, C_in] (``kd_conv2d_wgrad_x3``).  ``q_rows``: the first q_rows output channels ran
    with a folded 1 / 8 (the q rows of a qkv projection), and the gradient of the stored weight takes it too.  ``chunks`` = (patches per chunk,
    chunk count) overrides ``conv_wgrad_chunks`` (a test choosing its own cut of the sum).  ``bf16``: both operands rounded once to bf16, one
    bf16 MFMA per product with fp32 accumulation (``kd_conv2d_wgrad_bf16``, include/kdiff_unet_mixed.h) -- the same contract otherwise."""
    ldg, lda = _rows(g, "g"), _rows(a, "a")
    c_out, c_in = g.shape[1], a.shape[1]
    _tokens(g, B, H, W, "conv2d_wgrad")
    _tokens(a, B, H, W, "conv2d_wgrad")
    if out is None:
        if accumulate:
            raise ValueError("conv2d_wgrad: accumulate needs the tensor to add to (out)")
        out = torch.empty(c_out, c_in, ks, ks, device=g.device, dtype=torch.float32)
    elif tuple(_chk(out, "out").shape) != (c_out, c_in, ks, ks):
        raise ValueError(f"conv2d_wgrad: out {tuple(out.shape)} != {(c_out, c_in, ks, ks)}")
    per_chunk, nchunk = conv_wgrad_chunks(B, H, W, c_in, c_out) if chunks is None else chunks
    ws = torch.empty(max(nchunk, 1) * ks * ks * c_out * c_in, device=g.device, dtype=torch.float32)
    name = "kd_conv2d_wgrad_bf16" if bf16 else "kd_conv2d_wgrad_x3"
    nat.check(getattr(nat.lib(), name)(_p(g), ldg, _p(a), lda, _p(ws), _p(out), B, H, W, c_in, c_out, ks, int(q_rows), int(per_chunk), int(nchunk),
                                       int(bool(accumulate)), _stream()), name)
    return out


def adagn_wb_grad(x, stats, wb, g_y, gelu=False, out=None):
    """g_wb [B, 2 C] = the gradient of the (w, b) pair ``adagn_apply(x, stats, wb, gelu)`` reads from ``wb``, from the gradient g_y on its
    output (``kd_adagn_wb_grad_f32``).  ``out`` is usually the norm's column range of the call's gradient table."""
    ldx, ldgy, wbs, B, groups, hw, chan = _adagn_vjp_dims("adagn_wb_grad", x, stats, wb, g_y)
    out = torch.empty(B, 2 * chan, device=x.device, dtype=torch.float32) if out is None else out
    gws = _rows(out, "g_wb", 2 * chan)
    if out.shape[0] != B:
        raise ValueError(f"adagn_wb_grad: g_wb {tuple(out.shape)} != {(B, 2 * chan)}")
    nat.check(nat.lib().kd_adagn_wb_grad_f32(_p(x), ldx, _p(stats), _p(wb), wbs, _p(g_y), ldgy, _p(out), gws, B, hw, chan, groups, int(bool(gelu)),
                                             _stream()), "kd_adagn_wb_grad_f32")
    return out


def gelu_vjp(pre, g_y, out=None):
    """g_x = g_y gelu'(pre) for the exact (erf) GELU (``kd_gelu_vjp_f32``); ``out`` may be g_y."""
    if _chk(pre, "pre").shape != _chk(g_y, "g_y").shape:
        raise ValueError(f"gelu_vjp: g_y shape {tuple(g_y.shape)} != pre shape {tuple(pre.shape)}")
    out = torch.empty_like(pre) if out is None else out
    if _chk(out, "g_x").shape != pre.shape:
        raise ValueError(f"gelu_vjp: g_x shape {tuple(out.shape)} != pre shape {tuple(pre.shape)}")
    nat.check(nat.lib().kd_gelu_vjp_f32(_p(pre), _p(g_y), _p(out), pre.numel(), _stream()), "kd_gelu_vjp_f32")
    return out


def bias_grad(g, out=None, accumulate=False, q_cols=0):
    """The gradient of a convolution's bias: out [C] (+)= the column sums of the gradient g on its output -- token rows [B*H*W, C] with a row
    stride, or a contiguous NCHW image [B, C, H, W] (``kd_bias_grad_f32``).  ``q_cols``: the first q_cols sums take a folded 1 / 8."""
    if g.dim() == 4:
        rows, cols, ldg, nchw = g.shape[0] * g.shape[2] * g.shape[3], g.shape[1], 0, g.shape[2] * g.shape[3]
        _chk(g, "g")
    else:
        ldg, nchw = _rows(g, "g"), 0
        rows, cols = g.shape
    if out is None:
        if accumulate:
            raise ValueError("bias_grad: accumulate needs the tensor to add to (out)")
        out = torch.empty(cols, device=g.device, dtype=torch.float32)
    elif tuple(_chk(out, "out").shape) != (cols,):
        raise ValueError(f"bias_grad: out {tuple(out.shape)} != {(cols,)}")
    ws = torch.empty(-(-rows // 256) * cols, device=g.device, dtype=torch.float64)
    nat.check(nat.lib().kd_bias_grad_f32(_p(g), ldg, _p(ws), _p(out), rows, cols, nchw, int(q_cols), int(bool(accumulate)), _stream()),
              "kd_bias_grad_f32")
    return out


# ---- dropout of the training loss (csrc/unet_drop_f32.hip, csrc/conv_x3.hip, csrc/vjp_f32.hip; contracts: include/kdiff_unet_drop.h): what
# ``ImageDenoiserModelV1.loss_forward`` adds in training mode after ``enable_dropout()``.  With a rate of 0 nothing here is called: the walk takes
# no table and no key and launches what it launched before --------------------------------------------------------------------------------------------

def drop_factors(p):
    """(threshold, scale) of the mask contract for a rate p in (0, 1): keep iff word >= floor(p 2^32); a kept element times (float)(1 / (1 - p))."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"dropout rate {p} outside (0, 1)")
    return math.floor(p * 2.0 ** 32), 1.0 / (1.0 - p)


def _key(key):
    if _chk(key, "key", torch.int64).numel() != 1:
        raise ValueError(f"dropout: the key is one int64 (got {key.numel()} elements)")
    return _p(key)


def chan_layout(sites):
    """[(site id, column offset, C)] of the channel sites ``sites`` = [(site id, C)] in one table, and the table's width."""
    out, off = [], 0
    for site, chan in sites:
        out.append((int(site), off, int(chan)))
        off += int(chan)
    return out, off


def chan_mask(key, layout, B, p, sites_dev=None, out=None):
    """table [B, sum of C]: the factor (0 or 1 / (1 - p)) of every (sample, channel) of ALL channel sites of a loss call, one launch
    (``kd_chan_mask_f32``).  ``layout`` = ``chan_layout``'s triples; ``sites_dev``: the same triples as an int64 [n, 3] device tensor (built
    here when None; the walk keeps one per device)."""
    width = max((off + chan for _, off, chan in layout), default=0)
    if not layout or any(off < 0 or chan <= 0 or not 0 <= site < 1 << 63 for site, off, chan in layout):
        raise ValueError(f"chan_mask: layout {layout} is not a list of (site id, column offset, C)")
    threshold, scale = drop_factors(p)
    kp = _key(key)
    if sites_dev is None:
        sites_dev = torch.tensor(layout, dtype=torch.int64, device=key.device)
    if tuple(_chk(sites_dev, "sites", torch.int64).shape) != (len(layout), 3):
        raise ValueError(f"chan_mask: sites {tuple(sites_dev.shape)} != {(len(layout), 3)}")
    out = torch.empty(B, width, device=key.device, dtype=torch.float32) if out is None else out
    stride = _rows(out, "table")
    if out.shape[0] != B or out.shape[1] < width:
        raise ValueError(f"chan_mask: table {tuple(out.shape)} for batch {B} and {width} columns")
    nat.check(nat.lib().kd_chan_mask_f32(kp, _p(sites_dev), len(layout), threshold, scale, _p(out), stride, B, _stream()), "kd_chan_mask_f32")
    return out


def chan_scale(g, m, B, out=None):
    """out = g * m[b] per (sample, channel): the transpose of the channel mask on a gradient g [B*HW, C], m [B, C] a site's column range of the
    table (``kd_chan_scale_f32``).  ``out`` may be g (in place)."""
    ldg = _rows(g, "g")
    chan = g.shape[1]
    cs = _rows(m, "chan_scale", chan)
    if m.shape[0] != B or g.shape[0] % B:
        raise ValueError(f"chan_scale: chan_scale {tuple(m.shape)} / {g.shape[0]} rows for batch {B}")
    out = torch.empty(g.shape[0], chan, device=g.device, dtype=torch.float32) if out is None else out
    ldo = _rows(out, "out", chan)
    if out.shape[0] != g.shape[0]:
        raise ValueError("chan_scale: out has the rows of g")
    nat.check(nat.lib().kd_chan_scale_f32(_p(g), ldg, _p(m), cs, _p(out), ldo, B, g.shape[0] // B, chan, _stream()), "kd_chan_scale_f32")
    return out


def _attn_dims(qkv, nh):
    if _chk(qkv, "qkv").dim() != 3 or qkv.shape[2] != 3 * nh * 64:
        raise ValueError(f"attention with dropout: qkv is [B, T, 3 * {nh} * 64] (got {tuple(qkv.shape)})")
    return qkv.shape[0], qkv.shape[1]


def attn_global_drop(qkv, nh, key, site, p, out=None):
    """``ops.attn_global`` with dropout on the softmax probabilities (``kd_attn_global_drop_f32``): qkv [B, T, 3 nh 64] with the scale already
    in q -> [B, T, nh 64].  p == 0: ``ops.attn_global`` itself."""
    if not p:
        return ops.attn_global(qkv, nh, out=out)
    B, T = _attn_dims(qkv, nh)
    threshold, scale = drop_factors(p)
    out = torch.empty(B, T, nh * 64, device=qkv.device, dtype=torch.float32) if out is None else out
    if tuple(_chk(out, "out").shape) != (B, T, nh * 64):
        raise ValueError(f"attn_global_drop: out {tuple(out.shape)} != {(B, T, nh * 64)}")
    nat.check(nat.lib().kd_attn_global_drop_f32(_p(qkv), _p(out), B, T, nh, _key(key), int(site), threshold, scale, _stream()),
              "kd_attn_global_drop_f32")
    return out


def attn_global_drop_vjp(qkv, g_out, nh, key, site, p):
    """g_qkv of ``attn_global_drop`` from the gradient g_out [B, T, nh 64] on its output (``kd_attn_global_drop_vjp_f32``); the masks are
    regenerated from (key, site).  p == 0: ``ops.attn_global_vjp`` itself."""
    if not p:
        return ops.attn_global_vjp(qkv, g_out, nh)
    B, T = _attn_dims(qkv, nh)
    if tuple(_chk(g_out, "g_out").shape) != (B, T, nh * 64):
        raise ValueError(f"attn_global_drop_vjp: g_out {tuple(g_out.shape)} != {(B, T, nh * 64)}")
    threshold, scale = drop_factors(p)
    g = torch.empty_like(qkv)
    stats = torch.empty(2, B, nh, T, device=qkv.device, dtype=torch.float32)
    nat.check(nat.lib().kd_attn_global_drop_vjp_f32(_p(qkv), _p(g_out), _p(g), _p(stats[0]), _p(stats[1]), B, T, nh, _key(key), int(site), threshold,
                                                    scale, _stream()), "kd_attn_global_drop_vjp_f32")
    return g

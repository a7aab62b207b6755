"""The attention operators the reference's model calls into third-party libraries for, under THEIR names, signatures and tensor
layouts, on the HIP attention cores of this package -- the operator-level seam of SURVEY.md section 8b:

    natten.functional.na2d(q, k, v, kernel_size, scale=1.0)            image_transformer_v2.py:428     q, k, v [n, h, w, nh, e]
    flash_attn.flash_attn_qkvpacked_func(qkv, softmax_scale=1.0)       image_transformer_v2.py:383     qkv [n, s, 3, nh, e]
    F.scaled_dot_product_attention(q, k, v, scale=1.0)                 image_transformer_v2.py:392     q, k, v [n, nh, s, e]
    apply_window_attention(window_size, window_shift, q, k, v)         image_transformer_v2.py:319     q, k, v [n, nh, h, w, e]

A maintainer of the reference who wants only the attention cores swaps the import (``natten`` and ``flash_attn`` below are
the namespaces to import in place of the libraries); the model of this package does not come through here -- its qkv projection writes the
packed operand the cores read, with q and k already scaled and rotated.  What these wrappers add around a core is layout plumbing on the
device (one concatenation into the packed [.., 3 * nh * e] operand, the softmax scale folded into q); the arithmetic is the core's: fp32
tensors take the fp32-parity cores (``KDIFF_GEMM`` = split3 / exact decides which), bf16 tensors the bf16 cores.  Limits of the cores,
stated as errors: head dimension 64, dilation 1, no mask, no dropout, not causal.

Derivatives.  The operators are differentiable in both directions: when grad mode is on and q / k / v require grad, or when one of them
carries a forward-mode tangent (``torch.autograd.forward_ad``), the call goes through one ``torch.autograd.Function`` (``_Attention``);
otherwise it is the plain call, with nothing saved and nothing in the graph, and the forward output is the same bits either way.  The
backward and the tangent run on the fp32 reverse- and forward-mode attention kernels (csrc/vjp_f32.hip, csrc/jvp_f32.hip: ``ops.attn_*_vjp``
/ ``ops.attn_*_jvp``), whatever ``KDIFF_GEMM`` says and for every kernel size the forward takes.  For bf16 tensors the forward is the bf16
core's, the saved bf16 copy of q, k, v is widened to fp32 for the derivative kernels (the softmax scale folded in there, in fp32), and
the result is rounded to bf16 once at the end: the gradient of fp32 attention at the bf16-rounded inputs, not a bf16 backward.  First
derivatives only: a second backward raises.
"""
from types import SimpleNamespace

import torch
from torch.autograd import forward_ad
from torch.autograd.function import once_differentiable

from . import _native as nat
from . import ops

D_HEAD = 64


def _split_stored(x):
    """fp32 [..., C] -> the operand format of the split-bf16x3 attention cores (KdGemm.qkv_packed, include/kdiff_hip.h): every 4 values' 16
    bytes hold [hi: 4 x bf16][lo: 4 x bf16], hi = bf16(x), lo = bf16(x - hi).  In the model the qkv projection's epilogue writes this; here it
    is three elementwise torch ops on the device."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    both = torch.cat([hi.view(*x.shape[:-1], -1, 4), lo.view(*x.shape[:-1], -1, 4)], dim=-1)        # [..., C / 4, 8] bf16
    return both.view(torch.float32).view(x.shape)


def _check(q, what):
    if q.shape[-1] != D_HEAD:
        raise NotImplementedError(f"{what}: the HIP attention cores take head dimension {D_HEAD} (got {q.shape[-1]})")
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{what}: float32 or bfloat16 tensors (got {q.dtype})")
    if not q.is_cuda:
        raise RuntimeError(f"{what}: the HIP path needs tensors on a ROCm device (got {q.device}); there is no CPU fallback")


def _pack(q, k, v, scale, default_scale):
    """q, k, v [..., nh, e] -> the cores' packed operand [..., 3 * nh * e] (all q heads, all k heads, all v heads), q times the softmax scale."""
    scale = default_scale if scale is None else float(scale)
    if scale != 1.0:
        q = q * scale
    return torch.cat([q.flatten(-2), k.flatten(-2), v.flatten(-2)], dim=-1)


# ---- the three cores behind the operators: "na2d" (arg = kernel size), "window" (arg = (window size, shift)), "global" (arg = None) -----------

def _core(kind, packed, nh, arg):
    """Attention of the packed operand [.., 3 * nh * 64] -> [.., nh * 64] in the operand's dtype."""
    if kind == "na2d":
        if packed.dtype == torch.float32 and ops._prec_of(packed) == nat.PREC_SPLIT3:
            # the fp32-parity mode's neighbourhood core (every kernel size) reads split-stored operands
            return ops.attn_na2d(_split_stored(packed), nh, arg, prep="packed")
        if packed.dtype == torch.float32 and arg != 7:
            raise NotImplementedError("na2d: the exact-fp32 neighbourhood core takes kernel_size 7 only (KDIFF_GEMM=split3 and bf16 tensors: 3 .. 13)")
        return ops.attn_na2d(packed, nh, arg)
    if kind == "window":
        return ops.attn_window(packed, nh, *arg)
    return ops.attn_global(packed, nh)


def _core_vjp(kind, packed, g_out, nh, arg):
    """fp32 packed operand and the gradient on the output [.., nh * 64] -> the gradient on the packed operand."""
    if kind == "na2d":
        return ops.attn_na2d_vjp(packed, g_out, nh, arg)
    if kind == "window":
        return ops.attn_window_vjp(packed, g_out, nh, *arg)
    return ops.attn_global_vjp(packed, g_out, nh)


def _core_jvp(kind, packed, packed_dot, nh, arg):
    """fp32 packed operand and its tangent -> (output, tangent of the output) [.., nh * 64]."""
    if kind == "na2d":
        return ops.attn_na2d_jvp(packed, packed_dot, nh, arg)
    if kind == "window":
        return ops.attn_window_jvp(packed, packed_dot, nh, *arg)
    return ops.attn_global_jvp(packed, packed_dot, nh)


class _Attention(torch.autograd.Function):
    """One core on q, k, v ``[.., nh, 64]`` (heads last: the operators below bring their layouts here with views, which autograd carries back
    to the caller's layout) -> ``[.., nh, 64]``, differentiable in reverse and forward mode.  The forward is the plain call's: pack, then
    the core.  Saved for both directions is one tensor of our own, the concatenation [.., 3 * nh * 64] of q, k, v in the input dtype;
    neither the caller's q / k / v (the reference rotates q and k in place around these calls) nor the output.  The softmax scale is not
    in the saved copy: ``_operand32`` folds it into q after widening to fp32 -- for fp32 tensors the bits the core read, for bf16 tensors
    without the rounding of ``q * scale`` to bf16 that the bf16 core's operand has, so the derivative is taken at the caller's own q.  The
    backward is one launch of the fp32 reverse-mode kernels, the tangent one launch of the forward-mode kernels; each result is rounded
    to the input dtype once, at the end."""

    @staticmethod
    def forward(ctx, q, k, v, kind, arg, scale):
        packed = _pack(q, k, v, 1.0, 1.0)
        ctx.save_for_backward(packed)
        ctx.save_for_forward(packed)
        ctx.kind, ctx.arg, ctx.scale, ctx.nh = kind, arg, scale, q.shape[-2]
        return _core(kind, packed if scale == 1.0 else _pack(q, k, v, scale, 1.0), ctx.nh, arg).view(q.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        packed, = ctx.saved_tensors
        lead, nh = packed.shape[:-1], ctx.nh
        g_out = g_out.to(torch.float32).reshape(*lead, nh * D_HEAD).contiguous()
        g = _core_vjp(ctx.kind, _operand32(packed, nh, ctx.scale), g_out, nh, ctx.arg).view(*lead, 3, nh, D_HEAD)
        g_q, g_k, g_v = (g[..., t, :, :] if need else None for t, need in enumerate(ctx.needs_input_grad[:3]))
        if g_q is not None and ctx.scale != 1.0:
            g_q = g_q * ctx.scale
        return (*(None if t is None else t.to(packed.dtype) for t in (g_q, g_k, g_v)), None, None, None)

    @staticmethod
    def jvp(ctx, q_dot, k_dot, v_dot, *_):
        packed, = ctx.saved_tensors
        lead, nh = packed.shape[:-1], ctx.nh
        zeros = lambda: torch.zeros(*lead, nh, D_HEAD, device=packed.device)
        packed_dot = _pack(*(zeros() if t is None else t.float() for t in (q_dot, k_dot, v_dot)), ctx.scale, 1.0)
        _, o_dot = _core_jvp(ctx.kind, _operand32(packed, nh, ctx.scale), packed_dot, nh, ctx.arg)
        return o_dot.view(*lead, nh, D_HEAD).to(packed.dtype)


def _operand32(packed, nh, scale):
    """The saved concatenation of q, k, v -> the fp32 operand of the derivative kernels, q times the softmax scale."""
    packed = packed.float()
    if scale == 1.0:
        return packed
    return torch.cat([packed[..., :nh * D_HEAD] * scale, packed[..., nh * D_HEAD:]], dim=-1)


def _differentiated(*tensors):
    """Does this call need ``_Attention``: a graph to record, or a forward-mode tangent to carry?"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return True
    return any(forward_ad.unpack_dual(t).tangent is not None for t in tensors)


def _attention(q, k, v, kind, arg, scale):
    """q, k, v [.., nh, 64] -> [.., nh, 64] on the core ``kind``: the plain call, or ``_Attention`` when a derivative is wanted."""
    if _differentiated(q, k, v):
        return _Attention.apply(q, k, v, kind, arg, scale)
    return _core(kind, _pack(q, k, v, scale, 1.0), q.shape[-2], arg).view(q.shape)


def na2d(q, k, v, kernel_size, dilation=1, scale=None):
    """``natten.functional.na2d``: fused 2-D neighbourhood attention, q / k / v ``[n, h, w, heads, 64]`` -> ``[n, h, w, heads, 64]``;
    every query attends the ``kernel_size`` x ``kernel_size`` keys of its clamped window; ``scale`` defaults to NATTEN's ``64 ** -0.5``
    (the reference passes 1.0: its q and k are cosine-sim scaled).  Odd kernel sizes 3 .. 13.  Differentiable (module docstring): the
    gradients and tangents come from the fp32 kernels at every kernel size, so the only kernel-size limit is the forward's."""
    _check(q, "na2d")
    if q.dim() != 5 or q.shape != k.shape or q.shape != v.shape:
        raise ValueError(f"na2d: q, k, v must share the shape [n, h, w, heads, {D_HEAD}] (got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    if isinstance(kernel_size, (tuple, list)):
        if len(set(kernel_size)) != 1:
            raise NotImplementedError("na2d: square neighbourhoods only")
        kernel_size = kernel_size[0]
    if dilation not in (1, (1, 1), [1, 1]):
        raise NotImplementedError("na2d: dilation 1 only")
    return _attention(q, k, v, "na2d", int(kernel_size), D_HEAD ** -0.5 if scale is None else float(scale))


def flash_attn_qkvpacked_func(qkv, dropout_p=0.0, softmax_scale=None, causal=False):
    """``flash_attn.flash_attn_qkvpacked_func``: dense attention over the sequence, qkv ``[n, s, 3, heads, 64]`` -> ``[n, s, heads, 64]``;
    ``softmax_scale`` defaults to ``64 ** -0.5`` (the reference passes 1.0).  Differentiable (module docstring): the gradient comes back
    as one ``[n, s, 3, heads, 64]`` tensor."""
    _check(qkv, "flash_attn_qkvpacked_func")
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"flash_attn_qkvpacked_func: qkv must be [n, s, 3, heads, {D_HEAD}] (got {tuple(qkv.shape)})")
    if dropout_p or causal:
        raise NotImplementedError("flash_attn_qkvpacked_func: no dropout, not causal (the sampling path uses neither)")
    n, s, _, nh, e = qkv.shape
    scale = D_HEAD ** -0.5 if softmax_scale is None else float(softmax_scale)
    if _differentiated(qkv):
        return _Attention.apply(*qkv.unbind(2), "global", None, scale)
    if scale == 1.0:
        packed = qkv.reshape(n, s, 3 * nh * e)                   # already the cores' operand: "(t nh e)" with t outermost
    else:
        packed = _pack(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, 1.0)
    return ops.attn_global(packed.contiguous(), nh).view(n, s, nh, e)


def scaled_dot_product_attention(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None):
    """``torch.nn.functional.scaled_dot_product_attention`` for the global-attention call site: q / k / v ``[n, heads, s, 64]`` ->
    ``[n, heads, s, 64]``; ``scale`` defaults to ``1 / sqrt(64)`` (the reference passes 1.0).  The masked call of the shifted-window block
    (image_transformer_v2.py:333) is not this operator's job here: that block's windowing, roll and mask are inside ``ops.attn_window``
    (``apply_window_attention`` below).  Differentiable (module docstring)."""
    _check(query, "scaled_dot_product_attention")
    if attn_mask is not None or dropout_p or is_causal:
        raise NotImplementedError("scaled_dot_product_attention: no mask, no dropout, not causal (shifted windows: ops.attn_window)")
    if query.dim() != 4 or query.shape != key.shape or query.shape != value.shape:
        raise ValueError(f"scaled_dot_product_attention: q, k, v must share the shape [n, heads, s, {D_HEAD}]")
    scale = D_HEAD ** -0.5 if scale is None else float(scale)
    return _attention(query.transpose(1, 2), key.transpose(1, 2), value.transpose(1, 2), "global", None, scale).transpose(1, 2)


def apply_window_attention(window_size, window_shift, q, k, v, scale=None):
    """The reference's own ``apply_window_attention`` (image_transformer_v2.py:319-337): shifted-window attention, q / k / v
    ``[n, heads, H, W, 64]`` -> ``[n, heads, H, W, 64]``; ``scale`` defaults to SDPA's ``64 ** -0.5``.  The reference rolls, cuts windows,
    builds a mask and calls the masked SDPA; here all of that is inside ``ops.attn_window``.  Differentiable (module docstring).  Limits:
    ``window_size`` 4, 8 or 16, ``window_shift`` 0 or ``window_size // 2``, H and W multiples of ``window_size``."""
    _check(q, "apply_window_attention")
    if q.dim() != 5 or q.shape != k.shape or q.shape != v.shape:
        raise ValueError(f"apply_window_attention: q, k, v must share the shape [n, heads, H, W, {D_HEAD}]")
    if window_size not in (4, 8, 16):
        raise NotImplementedError(f"apply_window_attention: window_size 4, 8 or 16 (got {window_size})")
    if window_shift not in (0, window_size // 2):
        raise NotImplementedError(f"apply_window_attention: window_shift 0 or window_size // 2 (got {window_shift} with window_size {window_size})")
    H, W = q.shape[2:4]
    if H % window_size or W % window_size:
        raise NotImplementedError(f"apply_window_attention: H and W of q must be multiples of window_size (got H = {H}, W = {W} with window_size {window_size})")
    scale = D_HEAD ** -0.5 if scale is None else float(scale)
    heads_last = lambda t: t.permute(0, 2, 3, 1, 4)
    return _attention(heads_last(q), heads_last(k), heads_last(v), "window", (int(window_size), int(window_shift)), scale).permute(0, 3, 1, 2, 4)


def has_fused_na():
    """``natten.has_fused_na``: the fused operator is the only neighbourhood operator here, so the reference takes its ``na2d`` branch
    (image_transformer_v2.py:421)."""
    return True


# ``from k_diffusion_amd.compat import natten, flash_attn`` in place of the reference's ``import natten`` / ``import flash_attn`` (:19-27)
natten = SimpleNamespace(has_fused_na=has_fused_na, functional=SimpleNamespace(na2d=na2d))
flash_attn = SimpleNamespace(flash_attn_qkvpacked_func=flash_attn_qkvpacked_func)

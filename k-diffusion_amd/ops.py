"""Tensor-level wrappers over the C ABI (include/kdiff_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation below is a HIP
kernel from libkdiff_hip.so launched on ``torch.cuda.current_stream()``.  Tensors must be contiguous,
on a ROCm device and fp32 -- or, for the activation tensors of the bf16 arithmetic mode (``precision=PREC_BF16`` /
``KDIFF_GEMM=bf16``), bf16 -- anything else raises (there is no eager fallback).

The op names mirror the reference functions they replace
(k_diffusion/models/image_transformer_v2.py): ``rms_norm`` (:98), ``linear_geglu`` (:89),
``scale_for_cosine_sim``+``apply_rotary_emb_`` -> ``qk_prep_`` (:106, :230), SDPA / flash-attn ->
``attn_global`` (:383,:392), ``apply_window_attention`` -> ``attn_window`` (:319),
``natten.functional.na2d`` -> ``attn_na2d`` (:428).
"""
import ctypes as C
import os

import math

import torch

from . import _native as nat
from . import weights


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a tensor on a ROCm device (got {t.device}); there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_packed = weights.WeakCache()


def pack_weight(W, N, K, geglu, cache=True, bf16=False):
    """Packed image of a weight (uint8 tensor): the split-bf16 image of KD_PREC_SPLIT3, or with ``bf16=True`` the plain bf16
    image of KD_PREC_BF16, or with ``bf16="mx8"`` the e4m3 image + channel scales of kd_gemm_mx8 (``geglu`` 0 / 1 only).  ``geglu``: 0 / False plain, 1 / True GEGLU rows, 2 the k order of the fused FF block's down projection.  Weights are static while sampling, so the image is cached per tensor OBJECT
    (``weights.WeakCache``)."""
    geglu = int(geglu)

    def build():
        _chk(W, "W")
        lib = nat.lib()
        if bf16 == "mx8":
            size = lib.kd_packed_weight_bytes_mx8(N, K, geglu)
            if size <= 0:
                raise ValueError(f"kd_pack_weight_mx8: N={N} K={K} is not taken (K must be a multiple of 128)")
            img = torch.empty(size, device=W.device, dtype=torch.uint8)
            nat.check(lib.kd_pack_weight_mx8(_p(W), _p(img), N, K, geglu, _stream()), "kd_pack_weight_mx8")
        elif bf16:
            img = torch.empty(lib.kd_packed_weight_bytes_bf16(N, K, geglu), device=W.device, dtype=torch.uint8)
            nat.check(lib.kd_pack_weight_bf16(_p(W), _p(img), N, K, geglu, _stream()), "kd_pack_weight_bf16")
        else:
            img = torch.empty(lib.kd_packed_weight_bytes(N, K, geglu), device=W.device, dtype=torch.uint8)
            nat.check(lib.kd_pack_weight_bf16x3(_p(W), _p(img), N, K, geglu, _stream()), "kd_pack_weight_bf16x3")
        return img
    return _packed.get(W, (bf16 if bf16 == "mx8" else bool(bf16), geglu), (N, K), build, cache=cache)


def gemm(A, W, out, *, M, N, K, a_mode=nat.A_PLAIN, epi=nat.EPI_STORE, norm_scale=None, scale_stride=0,
         rows_per_sample=0, residual=None, grid=(0, 0), patch=(0, 0, 0), eps=1e-6, out_add=0.0,
         sigma=None, sigma_data=1.0, fac=None, scale_ptr=None, precision=None, qk=None, qkv_packed=False, per_row=False,
         a_planes=None, c_planes=None, launch=True, mx8=False, pack=pack_weight):
    """Fused GEMM (see KdGemm in include/kdiff_hip.h).  ``norm_scale`` may be a tensor or, with
    ``scale_ptr``, a raw device address inside a larger scale table.  ``precision``: nat.PREC_EXACT /
    nat.PREC_SPLIT3 / nat.PREC_BF16 (default: KDIFF_GEMM env, split3).  In bf16 mode A, out and residual are bf16 tensors
    (except the fp32 image side of the patch modes) and ``qk`` = (scale_h, rope_pos [T, 2], rope_freq [nh, 8], nh).
    ``per_row`` (fp32 modes): the per-row FMA kernel of the conditioning chain whatever M (KdGemm.per_row).
    ``a_planes`` / ``c_planes`` (split3): (hi, lo) bf16 tensors instead of the fp32 ``A`` / ``out`` (KdGemm.a_split / c_split; ``A`` / ``out``
    are then ignored and may be None).  ``launch=False``: only build and return the descriptor (for entry points that take one, e.g.
    kd_attn_block_bf16); ``A`` / ``out`` may then be None and ``scale_ptr`` 0, addresses the caller sets before each launch.
    ``pack``: the weight-image provider (``pack_weight``'s signature; the model's plans share one cache per model).  ``mx8`` (bf16
    tensors, norm -> store / qkv / GEGLU at K = 256 / 512): the product on the block-scaled fp8 matrix instruction (kd_gemm_mx8: e4m3
    weights with power-of-two channel scales, activations quantised per 32-k block)."""
    d = nat.KdGemm()
    d.per_row = 1 if per_row else 0
    d.precision = nat.kernel_precision() if precision is None else precision
    bf = d.precision == nat.PREC_BF16
    act = torch.bfloat16 if bf else torch.float32
    a_dt = torch.float32 if a_mode == nat.A_PATCH_NCHW else act
    c_dt = torch.float32 if epi == nat.EPI_UNPATCH_NCHW else act
    if mx8:
        if not bf:
            raise TypeError("mx8: bf16 activations only (precision=PREC_BF16)")
        d.Wp = pack(W, N, K, epi == nat.EPI_GEGLU, bf16="mx8").data_ptr()
    elif bf:
        d.Wp = pack(W, N, K, epi == nat.EPI_GEGLU, bf16=True).data_ptr()
    elif d.precision == nat.PREC_SPLIT3:
        d.Wp = pack(W, N, K, epi == nat.EPI_GEGLU).data_ptr()
    d.M, d.N, d.K = M, N, K
    d.a_mode, d.epi = a_mode, epi
    d.norm = 1 if (norm_scale is not None or scale_ptr is not None) else 0
    d.rows_per_sample, d.scale_stride = rows_per_sample, scale_stride
    d.gh, d.gw = grid
    d.ph, d.pw, d.chan = patch
    d.eps, d.out_add, d.sigma_data = eps, out_add, sigma_data
    d.W = _chk(W, "W").data_ptr()
    if a_planes is not None and mx8:          # (e4m3 rows [M, K], E8M0 block-scale bytes [M, K / 32]): kd_gemm_mx8's tiled form
        d.a_split, d.A, d.A_lo = 1, _chk(a_planes[0], "A e4m3", torch.uint8).data_ptr(), _chk(a_planes[1], "A scales", torch.uint8).data_ptr()
    elif a_planes is not None:
        d.a_split, d.A, d.A_lo = 1, _chk(a_planes[0], "A hi", torch.bfloat16).data_ptr(), _chk(a_planes[1], "A lo", torch.bfloat16).data_ptr()
    elif A is not None or launch:
        d.A = _chk(A, "A", a_dt).data_ptr()
    if c_planes is not None and mx8:          # the GEGLU result as (e4m3 rows [M, N], scale bytes [M, N / 32])
        d.c_split, d.C, d.C_lo = 1, _chk(c_planes[0], "C e4m3", torch.uint8).data_ptr(), _chk(c_planes[1], "C scales", torch.uint8).data_ptr()
        out = c_planes
    elif c_planes is not None:
        d.c_split, d.C, d.C_lo = 1, _chk(c_planes[0], "C hi", torch.bfloat16).data_ptr(), _chk(c_planes[1], "C lo", torch.bfloat16).data_ptr()
        out = c_planes
    elif out is not None or launch:
        d.C = _chk(out, "C", c_dt).data_ptr()
    d.R = None if residual is None else _chk(residual, "R", c_dt).data_ptr()
    d.scale = scale_ptr if scale_ptr is not None else (None if norm_scale is None else _chk(norm_scale, "scale").data_ptr())
    d.sigma = None if sigma is None else _chk(sigma, "sigma").data_ptr()
    d.fac = None if fac is None else _chk(fac, "fac").data_ptr()
    if qk is not None and bf:   # EPI_QKV, bf16 mode: (scale_h [nh], rope_pos [T, 2], rope_freq [nh, 8] in revolutions, nh)
        d.qk_scale, d.rope_pos, d.rope_freq = (_chk(t, n).data_ptr() for t, n in zip(qk[:3], ("qk_scale", "rope_pos", "rope_freq")))
        d.n_heads = qk[3]
    elif qk is not None:        # EPI_QKV: (scale_h [nh], cos [T, nh, 16], sin [T, nh, 16], nh)
        d.qk_scale, d.rope_cos, d.rope_sin = (_chk(t, n).data_ptr() for t, n in zip(qk[:3], ("qk_scale", "cos", "sin")))
        d.n_heads = qk[3]
        if len(qk) >= 6:        # + (rope_pos [T, 2], rope_freq [nh, 8] in revolutions): the round-3 split3 kernel evaluates the angles itself
            d.rope_pos, d.rope_freq = _chk(qk[4], "rope_pos").data_ptr(), _chk(qk[5], "rope_freq").data_ptr()
        d.qkv_packed = 1 if qkv_packed else 0      # q, k, v stored as split-bf16 chunks for the attention cores (prep="packed")
    if not launch:
        return d
    name = _gemm_entry(d.precision, mx8)
    nat.check(getattr(nat.lib(), name)(C.byref(d), _stream()), name)
    return out


def _gemm_entry(precision, mx8=False):        # entry point of a plain ``gemm`` descriptor
    return "kd_gemm_mx8" if mx8 else ("kd_gemm_bf16" if precision == nat.PREC_BF16 else "kd_gemm_f32")


def _prec_of(x):
    """Arithmetic mode implied by an activation tensor: bf16 tensors run the bf16 kernels, fp32 ones the KDIFF_GEMM fp32 mode."""
    if x.dtype == torch.bfloat16:
        return nat.PREC_BF16
    p = nat.kernel_precision()
    return nat.PREC_SPLIT3 if p == nat.PREC_BF16 else p


def linear(x, weight, residual=None, out=None, out_add=0.0):
    """x[..., K] @ weight[N, K]^T (+ residual)  --  Linear (:126-129) with the skip add fused."""
    K = x.shape[-1]
    M = x.numel() // K
    Nn = weight.shape[0]
    out = torch.empty(*x.shape[:-1], Nn, device=x.device, dtype=x.dtype) if out is None else out
    return gemm(x, weight, out, M=M, N=Nn, K=K, epi=nat.EPI_RESIDUAL if residual is not None else nat.EPI_STORE,
                residual=residual, out_add=out_add, precision=_prec_of(x))


def linear_geglu(x, weight, out=None):
    """linear_geglu (:89-95): value * gelu(gate), value = first half of the output features."""
    K = x.shape[-1]
    M = x.numel() // K
    d_ff = weight.shape[0] // 2
    out = torch.empty(*x.shape[:-1], d_ff, device=x.device, dtype=x.dtype) if out is None else out
    return gemm(x, weight, out, M=M, N=d_ff, K=K, epi=nat.EPI_GEGLU, precision=_prec_of(x))


def norm_split(x, scale=None, *, rows_per_sample=0, eps=1e-6):
    """AdaRMSNorm / RMSNorm (:98-103, :155-166) of fp32 rows -> (hi, lo) bf16 planes, the A operand of an ``a_planes`` GEMM.
    ``scale``: [B, K] per-sample, [K] shared, or None (plain split of ``x``)."""
    K = x.shape[-1]
    M = x.numel() // K
    hi, lo = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16), torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    stride = 0 if scale is None or scale.dim() == 1 else K
    nat.check(nat.lib().kd_norm_split_f32(_p(_chk(x, "x")), None if scale is None else _p(_chk(scale, "scale")), stride, rows_per_sample or M,
                                          _p(hi), _p(lo), M, K, eps, _stream()), "kd_norm_split_f32")
    return hi, lo


def rms_norm(x, scale, eps=1e-6, out=None):
    """rms_norm (:98-103) with a shared gain (RMSNorm :142-152)."""
    d = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    nat.check(nat.lib().kd_rmsnorm_f32(_p(_chk(x, "x")), _p(_chk(scale, "scale")), _p(_chk(out, "y")), x.numel() // d, d, eps, _stream()),
            "kd_rmsnorm_f32")
    return out


def norm_linear(x, scale, weight, *, rows_per_sample, epi=nat.EPI_STORE, out=None, eps=1e-6, qk=None, qkv_packed=False, mx8=False, c_fp8=False):
    """AdaRMSNorm/RMSNorm (:155-166) fused into the following Linear / LinearGEGLU.
    ``scale``: [B, K] per-sample scales (AdaRMSNorm: Linear(cond) + 1) or [K] shared gain.
    ``epi=EPI_QKV`` with ``qk=(scale_h, cos, sin, nh)``: qkv projection whose q, k come out prepared
    (scale_for_cosine_sim + apply_rotary_emb_, :106-121, :187-231), ready for the attention cores with prep=None."""
    K = x.shape[-1]
    M = x.numel() // K
    Nn = weight.shape[0] // (2 if epi == nat.EPI_GEGLU else 1)
    if c_fp8:            # mx8 + GEGLU: the result as (e4m3 rows [..., N] uint8, E8M0 scale bytes [..., N / 32] uint8) -- linear_mx8's A operand
        planes = (torch.empty(*x.shape[:-1], Nn, device=x.device, dtype=torch.uint8), torch.empty(*x.shape[:-1], Nn // 32, device=x.device, dtype=torch.uint8))
        return gemm(x, weight, None, M=M, N=Nn, K=K, epi=epi, norm_scale=scale, scale_stride=K if scale.dim() == 2 else 0,
                    rows_per_sample=rows_per_sample, eps=eps, precision=_prec_of(x), mx8=True, c_planes=planes)
    out = torch.empty(*x.shape[:-1], Nn, device=x.device, dtype=x.dtype) if out is None else out
    return gemm(x, weight, out, M=M, N=Nn, K=K, epi=epi, norm_scale=scale, scale_stride=K if scale.dim() == 2 else 0,
                rows_per_sample=rows_per_sample, eps=eps, qk=qk, qkv_packed=qkv_packed, precision=_prec_of(x), mx8=mx8)


def linear_mx8(a8, a_scales, weight, residual=None, out=None):
    """(e4m3 rows [..., K] uint8, E8M0 block-scale bytes [..., K / 32] uint8) @ e4m3(weight[N, K])^T (+ residual, bf16) -> bf16 [..., N]:
    kd_gemm_mx8's tiled form (the fp8 mode's down projection; both operands e4m3 on the block-scaled matrix instruction)."""
    K = a8.shape[-1]
    M = a8.numel() // K
    Nn = weight.shape[0]
    out = torch.empty(*a8.shape[:-1], Nn, device=a8.device, dtype=torch.bfloat16) if out is None else out
    return gemm(None, weight, out, M=M, N=Nn, K=K, epi=nat.EPI_RESIDUAL if residual is not None else nat.EPI_STORE, residual=residual,
                precision=nat.PREC_BF16, mx8=True, a_planes=(a8, a_scales))


def attn_block(x, scale, weight, *, rows_per_sample, qk, out=None, eps=1e-6):
    """The global-attention block as one launch (kd_attn_block_bf16; image_transformer_v2.py:370-392): x [B, T, K] bf16, ``scale`` [B, K]
    AdaRMSNorm scales, ``weight`` the qkv projection [3 K, K], ``qk`` = (scale_h [nh], rope_pos [T, 2], rope_freq [nh, 8] in revolutions, nh)
    -> attention output [B, T, K] bf16 (``out``).  256 tokens per sample, K = 64 nh in {256, 512}."""
    K = x.shape[-1]
    M = x.numel() // K
    out = torch.empty_like(x) if out is None else out
    d = gemm(x, weight, out, M=M, N=3 * K, K=K, epi=nat.EPI_QKV, norm_scale=scale, scale_stride=K, rows_per_sample=rows_per_sample, eps=eps,
             qk=qk, precision=nat.PREC_BF16, launch=False)
    nat.check(nat.lib().kd_attn_block_bf16(C.byref(d), _stream()), "kd_attn_block_bf16")
    return out


def proj_block(x, scale, weight, *, rows_per_sample, epi=nat.EPI_GEGLU, qk=None, out=None, eps=1e-6):
    """AdaRMSNorm -> wide projection in the attention block's form (kd_proj_block_bf16): the FF block's up projection + GEGLU
    (image_transformer_v2.py:487-491; ``weight`` [2 d_ff, K] -> [.., d_ff]) or, with ``epi=EPI_QKV`` and ``qk`` as in ``norm_linear``, the qkv
    projection with cosine-sim scale + RoPE (``weight`` [3 K, K] -> [.., 3 K]).  x [B, T, K] bf16 with T a multiple of 256, K in {256, 512};
    bit-identical to ``norm_linear(..., epi=epi)``."""
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0] // (2 if epi == nat.EPI_GEGLU else 1)
    out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=x.dtype) if out is None else out
    d = gemm(x, weight, out, M=M, N=N, K=K, epi=epi, norm_scale=scale, scale_stride=K, rows_per_sample=rows_per_sample, eps=eps, qk=qk,
             precision=nat.PREC_BF16, launch=False)
    nat.check(nat.lib().kd_proj_block_bf16(C.byref(d), _stream()), "kd_proj_block_bf16")
    return out


def token_merge(x, weight, out=None):
    """TokenMerge (:586-595) with the 2x2 space-to-depth folded into the GEMM's A addressing.  x: [B, 2h, 2w, C]."""
    B, H2, W2, Cc = x.shape
    h, w = H2 // 2, W2 // 2
    Nn = weight.shape[0]
    out = torch.empty(B, h, w, Nn, device=x.device, dtype=x.dtype) if out is None else out
    return gemm(x, weight, out, M=B * h * w, N=Nn, K=4 * Cc, a_mode=nat.A_MERGE2x2, grid=(h, w), precision=_prec_of(x))


def token_split_lerp(x, weight, skip, fac, out=None):
    """TokenSplit (:610-621): Linear -> depth-to-space -> lerp(skip, x, fac), fused.  x: [B, h, w, K]."""
    B, h, w, K = x.shape
    Nn = weight.shape[0]
    out = torch.empty_like(skip) if out is None else out
    return gemm(x, weight, out, M=B * h * w, N=Nn, K=K, epi=nat.EPI_SPLIT_LERP, residual=skip, fac=fac, grid=(h, w), precision=_prec_of(x))


def patch_in(image, weight, patch, sigma=None, sigma_data=1.0, out=None, precision=None):
    """NCHW->NHWC (:723) + TokenMerge(patch) (:672,:724) (+ Denoiser's x * c_in, layers.py:90).  The image is fp32; the tokens come
    out in the activation type of the arithmetic mode (bf16 for PREC_BF16)."""
    B, Cc, H, W = image.shape
    ph, pw = patch
    h, w = H // ph, W // pw
    Nn = weight.shape[0]
    precision = nat.kernel_precision() if precision is None else precision
    act = torch.bfloat16 if precision == nat.PREC_BF16 else torch.float32
    out = torch.empty(B, h, w, Nn, device=image.device, dtype=act) if out is None else out
    return gemm(image, weight, out, M=B * h * w, N=Nn, K=Cc * ph * pw, a_mode=nat.A_PATCH_NCHW, grid=(h, w),
                patch=(ph, pw, Cc), sigma=sigma, sigma_data=sigma_data, precision=precision)


def patch_out(x, norm_scale, weight, patch, channels, x_in=None, sigma=None, sigma_data=1.0, out=None, eps=1e-6):
    """out_norm (:758) + TokenSplitWithoutSkip (:759) + NHWC->NCHW (:760)
    (+ Denoiser's F * c_out + x * c_skip, layers.py:90).  x: [B, h, w, K]."""
    B, h, w, K = x.shape
    ph, pw = patch
    out = torch.empty(B, channels, h * ph, w * pw, device=x.device, dtype=torch.float32) if out is None else out
    return gemm(x, weight, out, M=B * h * w, N=channels * ph * pw, K=K, epi=nat.EPI_UNPATCH_NCHW, norm_scale=norm_scale,
                scale_stride=0, rows_per_sample=h * w, grid=(h, w), patch=(ph, pw, channels), residual=x_in, sigma=sigma,
                sigma_data=sigma_data, eps=eps, precision=_prec_of(x))


def ffn_supported(M, K, d_ff, bf16=True):
    """Does the fused feed-forward kernel take this shape (bf16 mode, or with ``bf16=False`` the fp32-parity split3 mode)?
    Otherwise use the up / down pair of ``gemm`` calls."""
    fn = nat.lib().kd_ffn_bf16_supported if bf16 else nat.lib().kd_ffn_f32_supported
    return bool(fn(int(M), int(K), int(d_ff)))


def ffn(x, norm_scale, w_up, w_down, out=None, scale_stride=None, rows_per_sample=None, eps=1e-6, attn=None, w_out=None, launch=True,
        pack=pack_weight):
    """FeedForwardBlock.forward (image_transformer_v2.py:487-493) in one kernel:
    out = x + down_proj(GEGLU(up_proj(rms_norm(x) * norm_scale))).  x: bf16 or fp32 [..., K]; norm_scale: fp32 [B, K] (one row per
    sample; ``rows_per_sample`` tokens each) ; w_up: fp32 [2 d_ff, K]; w_down: fp32 [K, d_ff].  ``out`` may be x.
    With ``attn`` ([..., K], the attention core's output, same dtype as x) and ``w_out`` ([K, K]) the attention block's out projection
    runs in front of the block in the same kernel: x' = x + attn @ w_out.T, out = x' + ff(x') (:473-476, :487-493); widths 128 (bf16,
    fp32) and 256 (fp32).  ``launch`` / ``pack`` as in ``gemm``: with ``launch=False`` only the descriptor is built and returned, and
    ``norm_scale`` may be None (the caller sets ``scale`` before each launch; ``scale_stride`` / ``rows_per_sample`` are then given)."""
    K = x.shape[-1]
    M = x.numel() // K
    d_ff = w_down.shape[1]
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("ffn: bf16 activations (KDIFF_GEMM=bf16) or fp32 activations (the fp32-parity split3 mode)")
    bf = x.dtype == torch.bfloat16
    out = torch.empty_like(x) if out is None else out
    d = nat.KdFfn()
    d.x, d.out = _p(_chk(x, "x", x.dtype)), _p(_chk(out, "out", x.dtype))
    if norm_scale is not None or launch:
        d.scale = _p(_chk(norm_scale, "norm_scale"))
    d.scale_stride = norm_scale.shape[-1] if scale_stride is None else scale_stride
    d.rows_per_sample = (M // max(norm_scale.numel() // norm_scale.shape[-1], 1)) if rows_per_sample is None else rows_per_sample
    d.eps = eps
    fused_out = attn is not None
    if fused_out and w_out is None:
        raise ValueError("ffn: attn and w_out go together")
    up_img, down_img = pack(w_up, d_ff, K, 3 if fused_out else 1, bf16=bf), pack(w_down, K, d_ff, 2, bf16=bf)
    d.Wp_up, d.Wp_down = _p(up_img), _p(down_img)
    d.M, d.K, d.d_ff = M, K, d_ff
    if fused_out:
        out_img = pack(w_out, K, K, 0, bf16=bf)
        d.attn, d.Wp_out = _p(_chk(attn, "attn", x.dtype)), _p(out_img)
    if not launch:
        return d
    name = "kd_ffn_bf16" if bf else "kd_ffn_f32"
    nat.check(getattr(nat.lib(), name)(C.byref(d), _stream()), name)
    return out


def attn_ffn_supported(batch, H, W, nh, kernel_size, K, d_ff):
    """Does the one-launch form of neighbourhood attention core + out projection + feed-forward block (``attn_ffn``) take this shape?"""
    return bool(nat.lib().kd_attn_ffn_f32_supported(int(batch), int(H), int(W), int(nh), int(kernel_size), int(K), int(d_ff)))


def attn_ffn(qkv, nh, kernel_size, x, norm_scale, w_up, w_down, w_out, out=None, eps=1e-6):
    """``ffn(x, ..., attn=attn_na2d(qkv, nh, kernel_size, prep="packed"), w_out=w_out)`` in ONE launch (fp32-parity split3 mode; the same
    bits): qkv fp32 [B, H, W, 3 nh 64] stored split by the qkv projection, x fp32 [B, H, W, K]; the attention rows never reach HBM.
    A shape ``attn_ffn_supported`` refuses is an error."""
    B, H, W = qkv.shape[0], qkv.shape[1], qkv.shape[2]
    out = torch.empty_like(x) if out is None else out
    d = ffn(x, norm_scale, w_up, w_down, out=out, rows_per_sample=H * W, eps=eps, attn=x, w_out=w_out, launch=False)
    d.attn = None
    nat.check(nat.lib().kd_attn_ffn_f32(_p(_chk(qkv, "qkv")), C.byref(d), B, H, W, nh, kernel_size, _stream()), "kd_attn_ffn_f32")
    return out


def fourier_sigma(sigma, weight, out=None):
    half = weight.shape[0]
    out = torch.empty(sigma.shape[0], 2 * half, device=sigma.device, dtype=torch.float32) if out is None else out
    nat.check(nat.lib().kd_fourier_sigma_f32(_p(_chk(sigma, "sigma")), _p(_chk(weight, "weight")), _p(_chk(out, "ff")), sigma.shape[0], half,
                                         _stream()), "kd_fourier_sigma_f32")
    return out


def fourier_features(x, weight, out=None):
    """FourierFeatures (k_diffusion/layers.py:285-293)."""
    half, in_dim = weight.shape
    B = x.numel() // in_dim
    out = torch.empty(*x.shape[:-1], 2 * half, device=x.device, dtype=torch.float32) if out is None else out
    nat.check(nat.lib().kd_fourier_f32(_p(_chk(x, "x")), _p(_chk(weight, "weight")), _p(_chk(out, "ff")), B, in_dim, half, _stream()), "kd_fourier_f32")
    return out


def cond_sum(a, b, emb=None, ids=None, c=None, out=None):
    """time_emb + aug_emb + class_emb + mapping_emb (:740)."""
    B, d = a.shape
    out = torch.empty_like(a) if out is None else out
    if emb is not None:
        _chk(ids, "ids", torch.int64)
    nat.check(nat.lib().kd_cond_sum_f32(_p(_chk(out, "out")), _p(_chk(a, "a")), _p(_chk(b, "b")), 1 if b.dim() == 2 else 0,
                                    _p(None if emb is None else _chk(emb, "emb")), _p(ids), _p(None if c is None else _chk(c, "c")),
                                    B, d, _stream()), "kd_cond_sum_f32")
    return out


def _qkv_dims(qkv, nh):
    if qkv.shape[-1] != 3 * nh * 64:
        raise ValueError(f"qkv last dim {qkv.shape[-1]} != 3*{nh}*64 (head dim is fixed at 64)")


def qk_prep_(qkv, scale_h, cos_t, sin_t, nh, eps=1e-6):
    """In place on qkv [B, T, 3*nh*64]: scale_for_cosine_sim (:106-114) + apply_rotary_emb_ (:230)."""
    _qkv_dims(qkv, nh)
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    nat.check(nat.lib().kd_qk_prep_f32(_p(_chk(qkv, "qkv")), _p(_chk(scale_h, "scale")), _p(_chk(cos_t, "cos")), _p(_chk(sin_t, "sin")),
                                   B, T, nh, eps, _stream()), "kd_qk_prep_f32")
    return qkv


def _prep_args(prep):
    if prep is None:
        return 0, None, None, None, 1e-6
    if isinstance(prep, str):
        if prep != "packed":
            raise ValueError("prep: None (q, k prepared), (scale_h, cos, sin[, eps]) or 'packed' (prepared and stored split by the qkv GEMM)")
        return 2, None, None, None, 1e-6
    scale_h, cos_t, sin_t = prep[:3]
    eps = prep[3] if len(prep) > 3 else 1e-6
    return 1, _p(_chk(scale_h, "scale")), _p(_chk(cos_t, "cos")), _p(_chk(sin_t, "sin")), eps


def _bf16_prep(prep):
    if prep is not None:
        raise ValueError("the bf16 attention cores take q, k already prepared by the qkv GEMM's epilogue (prep=None)")


def attn_global(qkv, nh, prep=None, out=None):
    """qkv: [B, T, 3*nh*64] -> [B, T, nh*64].  ``prep=(scale_h, cos, sin[, eps])`` applies the q/k
    preparation on the fly; ``None`` means q,k are already prepared."""
    _qkv_dims(qkv, nh)
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    out = torch.empty(*qkv.shape[:-1], nh * 64, device=qkv.device, dtype=qkv.dtype) if out is None else out
    if qkv.dtype == torch.bfloat16:
        _bf16_prep(prep)
        nat.check(nat.lib().kd_attn_global_bf16(_p(_chk(qkv, "qkv", torch.bfloat16)), _p(_chk(out, "out", torch.bfloat16)), B, T, nh, _stream()),
                  "kd_attn_global_bf16")
        return out
    f, s, c, sn, eps = _prep_args(prep)
    nat.check(nat.lib().kd_attn_global_f32(_p(_chk(qkv, "qkv")), _p(_chk(out, "out")), B, T, nh, f, s, c, sn, eps, _prec_of(qkv), _stream()), "kd_attn_global_f32")
    return out


def attn_window(qkv, nh, window_size, shift, prep=None, out=None):
    """qkv: [B, H, W, 3*nh*64] -> [B, H, W, nh*64]; apply_window_attention (:319-337)."""
    _qkv_dims(qkv, nh)
    B, H, W, _ = qkv.shape
    out = torch.empty(B, H, W, nh * 64, device=qkv.device, dtype=qkv.dtype) if out is None else out
    if qkv.dtype == torch.bfloat16:
        _bf16_prep(prep)
        nat.check(nat.lib().kd_attn_window_bf16(_p(_chk(qkv, "qkv", torch.bfloat16)), _p(_chk(out, "out", torch.bfloat16)), B, H, W, nh, window_size, shift,
                                                _stream()), "kd_attn_window_bf16")
        return out
    f, s, c, sn, eps = _prep_args(prep)
    nat.check(nat.lib().kd_attn_window_f32(_p(_chk(qkv, "qkv")), _p(_chk(out, "out")), B, H, W, nh, window_size, shift, f, s, c, sn, eps, _prec_of(qkv),
                                           _stream()), "kd_attn_window_f32")
    return out


def attn_na2d(qkv, nh, kernel_size, prep=None, out=None):
    """qkv: [B, H, W, 3*nh*64] -> [B, H, W, nh*64]; natten.functional.na2d(q, k, v, ks, scale=1.0) (:428)."""
    _qkv_dims(qkv, nh)
    B, H, W, _ = qkv.shape
    out = torch.empty(B, H, W, nh * 64, device=qkv.device, dtype=qkv.dtype) if out is None else out
    if qkv.dtype == torch.bfloat16:
        _bf16_prep(prep)
        nat.check(nat.lib().kd_attn_na2d_bf16(_p(_chk(qkv, "qkv", torch.bfloat16)), _p(_chk(out, "out", torch.bfloat16)), B, H, W, nh, kernel_size, _stream()),
                  "kd_attn_na2d_bf16")
        return out
    f, s, c, sn, eps = _prep_args(prep)
    nat.check(nat.lib().kd_attn_na2d_f32(_p(_chk(qkv, "qkv")), _p(_chk(out, "out")), B, H, W, nh, kernel_size, f, s, c, sn, eps, _prec_of(qkv), _stream()),
            "kd_attn_na2d_f32")
    return out


def sampler_step(op, x, den, in2=None, out=None, aux=None, c0=0.0, c1=0.0, c2=1.0, c3=0.0):
    out = torch.empty_like(den) if out is None else out
    for name, t in (("x", x), ("den", den), ("in2", in2), ("out", out), ("aux", aux)):
        if t is not None:
            _chk(t, name)
            if t.numel() != den.numel():
                raise ValueError(f"sampler_step: {name} has {t.numel()} elements, expected {den.numel()}")
    nat.check(nat.lib().kd_sampler_step_f32(op, _p(x), _p(den), _p(in2), _p(out), _p(aux), float(c0), float(c1), float(c2), float(c3),
                                        den.numel(), _stream()), "kd_sampler_step_f32")
    return out


def precond_in(x, sigma, sigma_data, out=None):
    out = torch.empty_like(x) if out is None else out
    B = x.shape[0]
    nat.check(nat.lib().kd_precond_in_f32(_p(_chk(x, "x")), _p(_chk(sigma, "sigma")), _p(_chk(out, "y")), float(sigma_data), B, x.numel() // B, _stream()),
            "kd_precond_in_f32")
    return out


def precond_out(f, x, sigma, sigma_data, out=None):
    out = torch.empty_like(x) if out is None else out
    B = x.shape[0]
    nat.check(nat.lib().kd_precond_out_f32(_p(_chk(f, "f")), _p(_chk(x, "x")), _p(_chk(sigma, "sigma")), _p(_chk(out, "y")), float(sigma_data), B,
                                       x.numel() // B, _stream()), "kd_precond_out_f32")
    return out


def rows_affine(f, a, x=None, c=None, out=None):
    """y[b] = f[b] * a[b] (+ x[b] * c[b]): per-sample scalars over image-sized tensors (external.py forward()s)."""
    out = torch.empty_like(f) if out is None else out
    B = f.shape[0]
    nat.check(nat.lib().kd_rows_affine_f32(_p(_chk(f, "f")), _p(None if x is None else _chk(x, "x")), _p(_chk(a, "a")),
                                       _p(None if c is None else _chk(c, "c")), _p(_chk(out, "y")), B, f.numel() // B, _stream()),
            "kd_rows_affine_f32")
    return out


def sigma_to_t(sigma, log_sigmas, quantize):
    out = torch.empty(sigma.shape, device=sigma.device, dtype=torch.float32)
    nat.check(nat.lib().kd_sigma_to_t_f32(_p(_chk(sigma.contiguous(), "sigma")), _p(_chk(log_sigmas, "log_sigmas")), _p(out), sigma.numel(),
                                      log_sigmas.numel(), int(bool(quantize)), _stream()), "kd_sigma_to_t_f32")
    return out


def t_to_sigma(t, log_sigmas):
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    nat.check(nat.lib().kd_t_to_sigma_f32(_p(_chk(t.contiguous(), "t")), _p(_chk(log_sigmas, "log_sigmas")), _p(out), t.numel(), log_sigmas.numel(),
                                      _stream()), "kd_t_to_sigma_f32")
    return out


def dpm_eps(x, denoised, sigma, out=None):
    """(x - denoised) / sigma -- DPMSolver.eps (sampling.py:354), the reference's rounding order."""
    out = torch.empty_like(x) if out is None else out
    nat.check(nat.lib().kd_dpm_eps_f32(_p(_chk(out, "out")), _p(_chk(x, "x")), _p(_chk(denoised, "denoised")), float(sigma), x.numel(), _stream()),
              "kd_dpm_eps_f32")
    return out


def dpm_combine(x, eps, a, eps_r=None, b=0.0, out=None):
    """x - a * eps [- b * (eps_r - eps)]: every DPM-Solver state (sampling.py:363-387), the reference's rounding order."""
    out = torch.empty_like(x) if out is None else out
    nat.check(nat.lib().kd_dpm_combine_f32(_p(_chk(out, "out")), _p(_chk(x, "x")), _p(_chk(eps, "eps")), None if eps_r is None else _p(_chk(eps_r, "eps_r")),
                                           float(a), float(b), x.numel(), _stream()), "kd_dpm_combine_f32")
    return out


def dpm_error(x_low, x_high, x_prev, atol, rtol):
    """Adaptive DPM-Solver local error (sampling.py:464-465) as a python float: sqrt(sum(((lo - hi) / delta)^2) / numel).
    One launch writes fixed-grid partial sums; their total is taken on the host (the controller needs the value there)."""
    part = torch.empty(nat.lib().kd_dpm_error_partials(), device=x_low.device, dtype=torch.float32)
    nat.check(nat.lib().kd_dpm_error_f32(_p(_chk(x_low, "x_low")), _p(_chk(x_high, "x_high")), _p(_chk(x_prev, "x_prev")), float(atol), float(rtol),
                                         x_low.numel(), _p(part), _stream()), "kd_dpm_error_f32")
    return math.sqrt(float(part.double().sum().item()) / x_low.numel())


def brownian(out, seeds, T0, T1, t0, t1, mult, depth=36):
    """out[b, ...] = (W_b(t1) - W_b(t0)) * mult, one virtual Brownian tree per batch item (seeds: uint64 [B])."""
    B = out.shape[0]
    _chk(seeds, "seeds", torch.int64)
    nat.check(nat.lib().kd_brownian_f32(_p(_chk(out, "out")), _p(seeds), B, out.numel() // B, float(T0), float(T1), float(t0), float(t1),
                                    float(mult), depth, _stream()), "kd_brownian_f32")
    return out


def brownian_cached(out, w0, have0, w1, have1, seeds, T0, T1, t0, t1, mult, depth=36):
    """As ``brownian`` with the end-point tensors W(t0) / W(t1) kept by the caller: ``have*`` says the
    buffer already holds that end point (read, no descent); otherwise it is computed and stored."""
    B = out.shape[0]
    _chk(seeds, "seeds", torch.int64)
    for w in (w0, w1):
        if w is not None and _chk(w, "w").numel() != out.numel():
            raise ValueError("end-point buffers must match out")
    nat.check(nat.lib().kd_brownian_cached_f32(_p(_chk(out, "out")), _p(w0) if w0 is not None else None, _p(w1) if w1 is not None else None,
                                           int(bool(have0)), int(bool(have1)), _p(seeds), B, out.numel() // B, float(T0), float(T1),
                                           float(t0), float(t1), float(mult), depth, _stream()), "kd_brownian_cached_f32")
    return out


def randn_indexed(out, seeds, draw=0, scale=1.0):
    """out[b, ...] = scale * standard normals that are a function of (seeds[b], draw, element index) only (seeds: int64 [B] on the
    device, ``draw`` numbers the calls of one run): the device-side form of ``torch.randn(...) * sigma_max`` (sample.py:59) /
    ``randn_like`` (sampling.py:61-62) for jobs whose image i must not depend on the batch or rank it is drawn in."""
    B = out.shape[0]
    _chk(seeds, "seeds", torch.int64)
    if seeds.numel() != B:
        raise ValueError(f"one seed per batch item: {seeds.numel()} seeds for batch {B}")
    nat.check(nat.lib().kd_randn_f32(_p(_chk(out, "out")), _p(seeds), B, out.numel() // B, int(draw), float(scale), _stream()), "kd_randn_f32")
    return out


def to_uint8(x, out=None):
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8) if out is None else out
    if x.numel() == 0:       # an empty shard (more ranks than images in a round): nothing to launch, and the other ranks still gather
        _chk(x, "x"), _chk(out, "y", torch.uint8)
        return out
    nat.check(nat.lib().kd_to_uint8(_p(_chk(x, "x")), _p(_chk(out, "y", torch.uint8)), x.numel(), _stream()), "kd_to_uint8")
    return out


# ---- forward-mode (tangent) ops of the dual pass (log_likelihood; csrc/jvp_f32.hip).  fp32 tensors only: the dual pass is fp32 whatever
# KDIFF_GEMM says.  Each takes the primal and its tangent and returns both.

def rms_norm_jvp(x, x_dot, scale, rows_per_sample=None, eps=1e-6):
    """rms_norm / AdaRMSNorm (:98-103, :155-166) and its tangent.  x, x_dot: [..., d]; ``scale``: [d] shared gain, or [B, d] per-sample
    AdaRMSNorm scales with ``rows_per_sample`` rows each."""
    d = x.shape[-1]
    rows = x.numel() // d
    y, yd = torch.empty_like(x), torch.empty_like(x)
    stride = 0 if scale.dim() == 1 else scale.shape[-1]
    rps = rows if stride == 0 else (rows_per_sample or rows // scale.shape[0])
    nat.check(nat.lib().kd_rmsnorm_jvp_f32(_p(_chk(x, "x")), _p(_chk(x_dot, "x_dot")), _p(_chk(scale, "scale")), stride, rps, _p(y), _p(yd), rows, d,
                                           float(eps), _stream()), "kd_rmsnorm_jvp_f32")
    return y, yd


def geglu_jvp(h, h_dot):
    """linear_geglu's gate (:89-95) on a projection [..., 2 d_ff] (value first) and its tangent -> ([..., d_ff], [..., d_ff])."""
    d_ff = h.shape[-1] // 2
    rows = h.numel() // h.shape[-1]
    y = torch.empty(*h.shape[:-1], d_ff, device=h.device, dtype=torch.float32)
    yd = torch.empty_like(y)
    nat.check(nat.lib().kd_geglu_jvp_f32(_p(_chk(h, "h")), _p(_chk(h_dot, "h_dot")), _p(y), _p(yd), rows, d_ff, _stream()), "kd_geglu_jvp_f32")
    return y, yd


def qk_prep_jvp_(qkv, qkv_dot, scale_h, cos_t, sin_t, nh, eps=1e-6):
    """``qk_prep_`` (:106-121, :187-231) in place on qkv [B, ..., 3*nh*64] and on its tangent."""
    _qkv_dims(qkv, nh)
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    nat.check(nat.lib().kd_qk_prep_jvp_f32(_p(_chk(qkv, "qkv")), _p(_chk(qkv_dot, "qkv_dot")), _p(_chk(scale_h, "scale")), _p(_chk(cos_t, "cos")),
                                           _p(_chk(sin_t, "sin")), B, T, nh, float(eps), _stream()), "kd_qk_prep_jvp_f32")
    return qkv, qkv_dot


def _attn_jvp_out(qkv, qkv_dot, nh, out=None, out_dot=None):
    _qkv_dims(qkv, nh)
    if qkv_dot.shape != qkv.shape:
        raise ValueError(f"tangent shape {tuple(qkv_dot.shape)} != primal shape {tuple(qkv.shape)}")
    _chk(qkv, "qkv"), _chk(qkv_dot, "qkv_dot")
    shape = (*qkv.shape[:-1], nh * 64)
    out = torch.empty(shape, device=qkv.device, dtype=torch.float32) if out is None else out
    out_dot = torch.empty(shape, device=qkv.device, dtype=torch.float32) if out_dot is None else out_dot
    if tuple(_chk(out, "out").shape) != shape or tuple(_chk(out_dot, "out_dot").shape) != shape:
        raise ValueError(f"out {tuple(out.shape)} and out_dot {tuple(out_dot.shape)} must be {shape}")
    return out, out_dot


def attn_global_jvp(qkv, qkv_dot, nh, out=None, out_dot=None):
    """Dense softmax attention (:383, :392) on prepared q, k and its tangent: qkv [B, T..., 3*nh*64] -> (o, o_dot) [B, T..., nh*64]."""
    out, od = _attn_jvp_out(qkv, qkv_dot, nh, out, out_dot)
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    nat.check(nat.lib().kd_attn_global_jvp_f32(_p(qkv), _p(qkv_dot), _p(out), _p(od), B, T, nh, _stream()), "kd_attn_global_jvp_f32")
    return out, od


def attn_window_jvp(qkv, qkv_dot, nh, window_size, shift):
    """Shifted-window attention (:253-337) and its tangent: qkv [B, H, W, 3*nh*64]."""
    out, od = _attn_jvp_out(qkv, qkv_dot, nh)
    B, H, W, _ = qkv.shape
    nat.check(nat.lib().kd_attn_window_jvp_f32(_p(qkv), _p(qkv_dot), _p(out), _p(od), B, H, W, nh, window_size, shift, _stream()),
              "kd_attn_window_jvp_f32")
    return out, od


def attn_na2d_jvp(qkv, qkv_dot, nh, kernel_size):
    """Neighbourhood attention (natten na2d, :428; clamped window) and its tangent: qkv [B, H, W, 3*nh*64]."""
    out, od = _attn_jvp_out(qkv, qkv_dot, nh)
    B, H, W, _ = qkv.shape
    nat.check(nat.lib().kd_attn_na2d_jvp_f32(_p(qkv), _p(qkv_dot), _p(out), _p(od), B, H, W, nh, kernel_size, _stream()), "kd_attn_na2d_jvp_f32")
    return out, od



# ---- reverse-mode (vector-Jacobian) ops of the backward pass (gradients w.r.t. the input; csrc/vjp_f32.hip).  fp32 tensors only, whatever
# KDIFF_GEMM says.  Each takes the primal input of the piece and the gradient on its output and returns the gradient on its input.

def rms_norm_vjp(x, g_y, scale, rows_per_sample=None, eps=1e-6, add=None, out=None):
    """Input gradient of rms_norm / AdaRMSNorm (:98-103, :155-166), ``scale`` as in ``rms_norm_jvp`` and held fixed.  ``add``: a gradient
    to add to the result (what a residual add passes through); ``out`` may be ``add``."""
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty_like(x) if out is None else out
    stride = 0 if scale.dim() == 1 else scale.shape[-1]
    rps = rows if stride == 0 else (rows_per_sample or rows // scale.shape[0])
    for name, t in (("g_y", g_y), ("add", add), ("out", out)):
        if t is not None and _chk(t, name).shape != x.shape:
            raise ValueError(f"rms_norm_vjp: {name} shape {tuple(t.shape)} != x shape {tuple(x.shape)}")
    nat.check(nat.lib().kd_rmsnorm_vjp_f32(_p(_chk(x, "x")), _p(g_y), _p(_chk(scale, "scale")), stride, rps, _p(add), _p(out), rows, d, float(eps),
                                           _stream()), "kd_rmsnorm_vjp_f32")
    return out


def geglu_vjp(h, g_y, dropout=None):
    """Gradient of linear_geglu's gate (:89-95): the projection h [..., 2 d_ff] (value first) and the gradient on its output [..., d_ff]
    -> the gradient on h [..., 2 d_ff].  ``dropout`` = (key, site, p): the output went through ``dropout`` at that site, so g_y is masked
    first, inside the kernel (the same bits as ``dropout`` on g_y, then this)."""
    d_ff = h.shape[-1] // 2
    rows = h.numel() // h.shape[-1]
    if _chk(g_y, "g_y").numel() != rows * d_ff:
        raise ValueError(f"geglu_vjp: g_y has {g_y.numel()} elements, expected {rows * d_ff}")
    out = torch.empty_like(h)
    drop = _dropout_args(dropout)
    if drop is None:
        nat.check(nat.lib().kd_geglu_vjp_f32(_p(_chk(h, "h")), _p(g_y), _p(out), rows, d_ff, _stream()), "kd_geglu_vjp_f32")
    else:
        nat.check(nat.lib().kd_geglu_vjp_drop_f32(_p(_chk(h, "h")), _p(g_y), _p(out), rows, d_ff, *drop, _stream()), "kd_geglu_vjp_drop_f32")
    return out


def qk_prep_vjp_(qkv, g_qkv, scale_h, cos_t, sin_t, nh, eps=1e-6):
    """Transpose of ``qk_prep_`` (:106-121, :187-231) at the unprepared ``qkv``: ``g_qkv`` (same layout) holds the gradient w.r.t. the
    prepared q, k and is rewritten in place with the gradient w.r.t. the unprepared ones; its v part passes through."""
    _qkv_dims(qkv, nh)
    if _chk(g_qkv, "g_qkv").shape != qkv.shape:
        raise ValueError(f"qk_prep_vjp_: gradient shape {tuple(g_qkv.shape)} != qkv shape {tuple(qkv.shape)}")
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    nat.check(nat.lib().kd_qk_prep_vjp_f32(_p(_chk(qkv, "qkv")), _p(g_qkv), _p(_chk(scale_h, "scale")), _p(_chk(cos_t, "cos")), _p(_chk(sin_t, "sin")),
                                           B, T, nh, float(eps), _stream()), "kd_qk_prep_vjp_f32")
    return g_qkv


def _attn_vjp_bufs(qkv, g_out, nh):
    _qkv_dims(qkv, nh)
    _chk(qkv, "qkv"), _chk(g_out, "g_out")
    if g_out.shape != (*qkv.shape[:-1], nh * 64):
        raise ValueError(f"attention gradient shape {tuple(g_out.shape)} != output shape {(*qkv.shape[:-1], nh * 64)}")
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    stats = torch.empty(2, B, nh, T, device=qkv.device, dtype=torch.float32)       # per-query log-sum-exp, rowsum(dO * O)
    return torch.empty_like(qkv), stats[0], stats[1]


def attn_global_vjp(qkv, g_out, nh):
    """Gradient of dense softmax attention (:383, :392) on prepared q, k: qkv [B, T..., 3*nh*64], g_out [B, T..., nh*64] -> g_qkv."""
    g, lse, ds = _attn_vjp_bufs(qkv, g_out, nh)
    B = qkv.shape[0]
    T = qkv.numel() // (B * 3 * nh * 64)
    nat.check(nat.lib().kd_attn_global_vjp_f32(_p(qkv), _p(g_out), _p(g), _p(lse), _p(ds), B, T, nh, _stream()), "kd_attn_global_vjp_f32")
    return g


def attn_window_vjp(qkv, g_out, nh, window_size, shift):
    """Gradient of shifted-window attention (:253-337): qkv [B, H, W, 3*nh*64]."""
    g, lse, ds = _attn_vjp_bufs(qkv, g_out, nh)
    B, H, W, _ = qkv.shape
    nat.check(nat.lib().kd_attn_window_vjp_f32(_p(qkv), _p(g_out), _p(g), _p(lse), _p(ds), B, H, W, nh, window_size, shift, _stream()),
              "kd_attn_window_vjp_f32")
    return g


def attn_na2d_vjp(qkv, g_out, nh, kernel_size):
    """Gradient of neighbourhood attention (natten na2d, :428; clamped window): qkv [B, H, W, 3*nh*64]."""
    g, lse, ds = _attn_vjp_bufs(qkv, g_out, nh)
    B, H, W, _ = qkv.shape
    nat.check(nat.lib().kd_attn_na2d_vjp_f32(_p(qkv), _p(g_out), _p(g), _p(lse), _p(ds), B, H, W, nh, kernel_size, _stream()), "kd_attn_na2d_vjp_f32")
    return g


def precond_vjp(g, g_coef, sigma, sigma_data, h=None, h_coef=nat.PC_ONE, out=None):
    """coef(g_coef) * g (+ coef(h_coef) * h) per sample, coef one of the Karras scalings nat.PC_ONE / PC_SKIP / PC_OUT / PC_IN of sigma [B]
    (layers.py:70-74): the transposes of the preconditioning D = F(x c_in) c_out + x c_skip."""
    out = torch.empty_like(g) if out is None else out
    B = g.shape[0]
    for name, t in (("h", h), ("out", out)):
        if t is not None and _chk(t, name).shape != g.shape:
            raise ValueError(f"precond_vjp: {name} shape {tuple(t.shape)} != g shape {tuple(g.shape)}")
    if _chk(sigma, "sigma").numel() != B:
        raise ValueError(f"precond_vjp: {sigma.numel()} sigmas for batch {B}")
    nat.check(nat.lib().kd_precond_vjp_f32(_p(_chk(g, "g")), int(g_coef), _p(h), int(h_coef), _p(sigma), float(sigma_data), _p(out), B, g.numel() // B,
                                           _stream()), "kd_precond_vjp_f32")
    return out


# ---- parameter gradients and the training loss (csrc/wgrad_f32.hip; models/vjp.py, layers.Denoiser.loss).  fp32 arithmetic in every KDIFF_GEMM
# mode; every sum runs in a fixed order through a workspace (no atomics), so repeat calls give the same bits.

WGRAD_BLOCKS = 1024          # workgroups a weight-gradient GEMM aims at (row chunks x output tiles); the chunking is a function of the shape
WGRAD_BF16_BLOCKS = 512      # the same for the bf16 form's 128 x 128 tiles (two workgroups per CU)
WGRAD_BF16 = 2               # kd_wgrad_f32's arithmetic selector: 0 exact, 1 split3, 2 bf16 operands


DROPOUT_SITE = 1 << 62                # include/kdiff_hip.h: every dropout site id has this bit; the Brownian / randn counters never do


def _dropout_args(dropout):
    """(key pointer, site, threshold, scale) of the kernels' mask contract for ``dropout`` = (key, site, p), or None when nothing is
    dropped (None or p == 0).  key: a one-element int64 device tensor; p in [0, 1)."""
    if dropout is None:
        return None
    key, site, p = dropout
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout rate {p} outside [0, 1)")
    if p == 0.0:
        return None
    if _chk(key, "key", torch.int64).numel() != 1:
        raise ValueError(f"dropout: the key is one int64 (got {key.numel()} elements)")
    if not 0 <= int(site) < 1 << 64:
        raise ValueError(f"dropout: site {site} is not a 64-bit unsigned id")
    return _p(key), int(site), math.floor(p * 2.0 ** 32), 1.0 / (1.0 - p)


def dropout(x, key, site, p, out=None):
    """The training loss's dropout at one site (include/kdiff_hip.h, mask contract): out = x * m, m = scale or 0 from the counter-based
    mask of (key, site, element).  ``out`` may be ``x`` (in place).  p == 0 launches nothing (returns x, or out holding a copy of x)."""
    if out is not None and _chk(out, "out").shape != _chk(x, "x").shape:
        raise ValueError(f"dropout: out shape {tuple(out.shape)} != {tuple(x.shape)}")
    drop = _dropout_args((key, site, p))
    if drop is None:
        if out is None or out is x:
            return x
        return out.copy_(x)
    out = torch.empty_like(_chk(x, "x")) if out is None else out
    if x.numel():
        nat.check(nat.lib().kd_dropout_f32(_p(x), _p(out), x.numel(), *drop, _stream()), "kd_dropout_f32")
    return out


def wgrad_chunks(M, N, K):
    """(chunk_rows, nchunk) of ``kd_wgrad_f32``: a fixed function of the shape, so that the order of the sum is too."""
    tiles = -(-N // 64) * -(-K // 64)
    nchunk = max(1, min(-(-WGRAD_BLOCKS // tiles), -(-M // 64), 65535))
    chunk = -(-M // nchunk)
    chunk = -(-chunk // 32) * 32
    return chunk, -(-M // chunk)


def wgrad_chunks_bf16(M, N, K):
    """(chunk_rows, nchunk) of the bf16 form of ``kd_wgrad_f32`` (128 x 128 output tiles, steps of 32 rows): a function of the shape alone."""
    tiles = -(-N // 128) * -(-K // 128)
    nchunk = max(1, min(-(-WGRAD_BF16_BLOCKS // tiles), -(-M // 128), 65535))
    chunk = -(-M // nchunk)
    chunk = -(-chunk // 32) * 32
    return chunk, -(-M // chunk)


def wgrad(G, A, *, N=None, K=None, out=None, accumulate=False, gather=None, gather_geom=None, geglu=False, row_scale=None, col_scale=None,
          rows_per_sample=None, alpha=None, precision=None, dropout=None, bf16=False):
    """Weight gradient of a projection: dW[N, K] (+)= alpha * sum_m G[m, n] * A[m, k] over the stored rows m of G and A.

    ``gather``: None, ("g" | "a", nat.WG_MERGE2x2 | nat.WG_PATCH_NCHW) -- that operand is read through the 2x2 token merge of a fine NHWC
    grid or the patch gather of an NCHW image; ``gather_geom`` = (gh, gw, ph, pw, chan) of its coarse rows.  A's prologue: ``geglu`` (A
    holds [value | gate] rows; the operand is value * gelu(gate)), ``row_scale`` [M] and ``col_scale`` ([K] shared or [B, K] per sample of
    ``rows_per_sample`` rows).  ``alpha``: a one-element device tensor multiplying the result.  Arithmetic: the backward pass's rule --
    split3 on the matrix cores under KDIFF_GEMM split3 / bf16 / fp8, fp32 FMAs under exact (``precision`` overrides).  ``dropout`` =
    (key, site, p): A's plain [M, K] operand (after the GEGLU prologue) is masked as ``dropout`` masks that site; p == 0 is the plain
    call.  ``bf16`` (opt-in, whatever ``precision`` and KDIFF_GEMM say): both operands are rounded to bf16 (nearest even) after their whole
    prologue -- gather, GEGLU, dropout mask, row and column scale -- and every product is one bf16 MFMA with fp32 accumulation, the
    arithmetic of a ``Linear`` backward under the reference's ``--mixed-precision bf16``."""
    g_mode = a_mode = nat.WG_PLAIN
    gh = gw = ph = pw = chan = 0
    if gather is not None:
        which, mode = gather
        gh, gw, ph, pw, chan = gather_geom
        if which == "g":
            g_mode = mode
        else:
            a_mode = mode
    if g_mode == nat.WG_PLAIN:
        N = G.shape[-1] if N is None else N
        M = G.numel() // N
    if a_mode == nat.WG_PLAIN:
        K = (A.shape[-1] // 2 if geglu else A.shape[-1]) if K is None else K
        M = A.numel() // (2 * K if geglu else K)
    if g_mode != nat.WG_PLAIN:
        N = ph * pw * chan
    if a_mode != nat.WG_PLAIN:
        K = ph * pw * chan
    if g_mode == nat.WG_PLAIN and G.numel() != M * N:
        raise ValueError(f"wgrad: G has {G.numel()} elements, expected {M} x {N}")
    if a_mode == nat.WG_PLAIN and A.numel() != M * (2 * K if geglu else K):
        raise ValueError(f"wgrad: A has {A.numel()} elements, expected {M} rows of {2 * K if geglu else K}")
    if gather is not None:
        gathered = G if g_mode != nat.WG_PLAIN else A
        if gathered.numel() != M * ph * pw * chan or M % (gh * gw):
            raise ValueError(f"wgrad: gathered operand has {gathered.numel()} elements for {M} rows of {ph * pw * chan}")
    col_stride = 0
    if col_scale is not None:
        _chk(col_scale, "col_scale")
        col_stride = 0 if col_scale.dim() == 1 else K
        if col_scale.shape[-1] != K:
            raise ValueError(f"wgrad: col_scale has {col_scale.shape[-1]} columns, expected {K}")
        if col_stride and rows_per_sample is None:
            rows_per_sample = M // col_scale.shape[0]
    if row_scale is not None and _chk(row_scale, "row_scale").numel() != M:
        raise ValueError(f"wgrad: row_scale has {row_scale.numel()} elements for {M} rows")
    if out is None:
        if accumulate:
            raise ValueError("wgrad: accumulate needs out")
        out = torch.empty(N, K, device=G.device, dtype=torch.float32)
    elif _chk(out, "out").shape != (N, K):
        raise ValueError(f"wgrad: out shape {tuple(out.shape)} != {(N, K)}")
    if bf16:
        arith = WGRAD_BF16
        chunk, nchunk = wgrad_chunks_bf16(M, N, K)
    else:
        arith = int((_prec_of(G) if precision is None else precision) != nat.PREC_EXACT)
        chunk, nchunk = wgrad_chunks(M, N, K)
    ws = torch.empty(nchunk * N * K, device=G.device, dtype=torch.float32)
    args = (_p(_chk(G, "G")), g_mode, _p(_chk(A, "A")), a_mode, int(bool(geglu)), M, N, K, gh, gw, ph, pw, chan, _p(row_scale), _p(col_scale),
            col_stride, int(rows_per_sample or 1), _p(None if alpha is None else _chk(alpha, "alpha")), int(bool(accumulate)), arith, chunk,
            nchunk, _p(ws), _p(out))
    drop = _dropout_args(dropout)
    if drop is None:
        nat.check(nat.lib().kd_wgrad_f32(*args, _stream()), "kd_wgrad_f32")
    else:
        if a_mode != nat.WG_PLAIN:
            raise ValueError("wgrad: the dropout mask applies to plain A rows")
        bits = torch.empty((M * K + 31) // 32, device=G.device, dtype=torch.int32)
        nat.check(nat.lib().kd_wgrad_drop_f32(*args, *drop, _p(bits), _stream()), "kd_wgrad_drop_f32")
    return out


def row_rrms(x, eps=1e-6):
    """rsqrt(mean(x^2) + eps) per row of x [..., d] -> [rows]."""
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty(rows, device=x.device, dtype=torch.float32)
    nat.check(nat.lib().kd_row_rrms_f32(_p(_chk(x, "x")), _p(out), rows, d, float(eps), _stream()), "kd_row_rrms_f32")
    return out


def colsum(a, b=None, b2=None, row_scale=None, rows_per_seg=None, out=None, accumulate=False):
    """out[s, j] (+)= sum over the rows r of segment s of a[r, j] * (b[r, j] - b2[r, j]) * row_scale[r] (b, b2, row_scale optional);
    a [..., cols] -> [rows / rows_per_seg, cols] (one segment by default)."""
    cols = a.shape[-1]
    rows = a.numel() // cols
    rps = rows if rows_per_seg is None else rows_per_seg
    for name, t in (("b", b), ("b2", b2)):
        if t is not None and _chk(t, name).numel() != a.numel():
            raise ValueError(f"colsum: {name} has {t.numel()} elements, a has {a.numel()}")
    if row_scale is not None and _chk(row_scale, "row_scale").numel() != rows:
        raise ValueError(f"colsum: row_scale has {row_scale.numel()} elements for {rows} rows")
    if rows % rps:
        raise ValueError(f"colsum: {rows} rows are not segments of {rps}")
    nseg = rows // rps
    if out is None:
        if accumulate:
            raise ValueError("colsum: accumulate needs out")
        out = torch.empty(nseg, cols, device=a.device, dtype=torch.float32)
    elif _chk(out, "out").numel() != nseg * cols:
        raise ValueError(f"colsum: out has {out.numel()} elements, expected {nseg * cols}")
    ws = torch.empty(nseg * (-(-rps // 64)) * cols, device=a.device, dtype=torch.float32)
    nat.check(nat.lib().kd_colsum_f32(_p(_chk(a, "a")), _p(b), _p(b2), _p(row_scale), rows, cols, rps, int(bool(accumulate)), _p(ws), _p(out),
                                      _stream()), "kd_colsum_f32")
    return out


def attn_scale_grad(colsums, scale_h, nh, out=None, accumulate=False):
    """Gradient of the cosine-sim scale (:106-114) from ``colsum(g_prep, prep)`` over the tokens of a [.., 3 * nh * 64] qkv."""
    if _chk(colsums, "colsums").numel() != 3 * nh * 64:
        raise ValueError(f"attn_scale_grad: {colsums.numel()} column sums for {nh} heads")
    out = torch.empty(nh, device=colsums.device, dtype=torch.float32) if out is None else out
    nat.check(nat.lib().kd_attn_scale_grad_f32(_p(colsums), _p(_chk(scale_h, "scale")), nh, int(bool(accumulate)), _p(_chk(out, "out")), _stream()),
              "kd_attn_scale_grad_f32")
    return out


def class_emb_grad(g, ids, n_cls, out=None, accumulate=False):
    """Gradient of the class embedding table [n_cls, d] from the gradient g [B, d] on the looked-up rows; samples added in ascending order."""
    B, d = g.shape
    if _chk(ids, "ids", torch.int64).numel() != B:
        raise ValueError(f"class_emb_grad: {ids.numel()} ids for batch {B}")
    out = torch.empty(n_cls, d, device=g.device, dtype=torch.float32) if out is None else out
    nat.check(nat.lib().kd_class_emb_grad_f32(_p(_chk(g, "g")), _p(ids), B, d, n_cls, int(bool(accumulate)), _p(_chk(out, "out")), _stream()),
              "kd_class_emb_grad_f32")
    return out


def loss_prep(input, noise, sigma, sigma_data):
    """(noised, noised * c_in): the model input of Denoiser.loss (layers.py:78-81).  sigma: [B]."""
    B = input.shape[0]
    if _chk(noise, "noise").shape != _chk(input, "input").shape:
        raise ValueError(f"loss: noise shape {tuple(noise.shape)} != input shape {tuple(input.shape)}")
    noised, x_in = torch.empty_like(input), torch.empty_like(input)
    nat.check(nat.lib().kd_loss_prep_f32(_p(input), _p(noise), _p(_chk(sigma, "sigma")), float(sigma_data), _p(noised), _p(x_in), B, input.numel() // B,
                                         _stream()), "kd_loss_prep_f32")
    return noised, x_in


def loss(f, input, noised, sigma, sigma_data, weighting, c_weight=None):
    """Per-sample losses [B] = mean((f - target)^2) * c_weight, target = (input - c_skip noised) / c_out (layers.py:82-85)."""
    B = input.shape[0]
    if _chk(f, "f").shape != input.shape:
        raise ValueError(f"loss: model output shape {tuple(f.shape)} != input shape {tuple(input.shape)}")
    out = torch.empty(B, device=f.device, dtype=torch.float32)
    nat.check(nat.lib().kd_loss_f32(_p(f), _p(_chk(input, "input")), _p(_chk(noised, "noised")), _p(_chk(sigma, "sigma")), float(sigma_data), int(weighting),
                                    _p(None if c_weight is None else _chk(c_weight, "c_weight")), _p(out), B, input.numel() // B, _stream()), "kd_loss_f32")
    return out


def loss_vjp(f, input, noised, sigma, sigma_data, weighting, g_loss, c_weight=None):
    """Gradient of ``loss`` w.r.t. the model output f from the gradient g_loss [B] on the losses."""
    B = input.shape[0]
    out = torch.empty_like(f)
    nat.check(nat.lib().kd_loss_vjp_f32(_p(_chk(f, "f")), _p(_chk(input, "input")), _p(_chk(noised, "noised")), _p(_chk(sigma, "sigma")), float(sigma_data),
                                        int(weighting), _p(None if c_weight is None else _chk(c_weight, "c_weight")), _p(_chk(g_loss, "g_loss")), _p(out),
                                        B, input.numel() // B, _stream()), "kd_loss_vjp_f32")
    return out

def ll_div(x, denoised, denoised_dot, v, sigma):
    """(d, d_ll): d = (x - D) / sigma (to_d, sampling.py:46) and d_ll[b] = sum_b v * (v - D_dot) / sigma_b.  sigma: [B] fp32."""
    B = x.shape[0]
    d = torch.empty_like(x)
    d_ll = torch.empty(B, device=x.device, dtype=torch.float32)
    for name, t in (("denoised", denoised), ("denoised_dot", denoised_dot), ("v", v)):
        if _chk(t, name).shape != x.shape:
            raise ValueError(f"ll_div: {name} shape {tuple(t.shape)} != x shape {tuple(x.shape)}")
    if _chk(sigma, "sigma").numel() != B:
        raise ValueError(f"ll_div: {sigma.numel()} sigmas for batch {B}")
    nat.check(nat.lib().kd_ll_div_f32(_p(_chk(x, "x")), _p(denoised), _p(denoised_dot), _p(v), _p(sigma), _p(d), _p(d_ll), B, x.numel() // B,
                                      _stream()), "kd_ll_div_f32")
    return d, d_ll


def gauss_logp(z, sigma, add=None):
    """[B]: add[b] + sum over sample b of log N(z; 0, sigma^2) (torch.distributions.Normal(0, sigma).log_prob(z).flatten(1).sum(1))."""
    B = z.shape[0]
    out = torch.empty(B, device=z.device, dtype=torch.float32)
    nat.check(nat.lib().kd_gauss_logp_f32(_p(_chk(z, "z")), float(sigma), None if add is None else _p(_chk(add, "add")), _p(out), B, z.numel() // B,
                                          _stream()), "kd_gauss_logp_f32")
    return out


def _rk_terms(ks, coeffs, n):
    if not 1 <= len(ks) <= 7 or len(ks) != len(coeffs):
        raise ValueError(f"1 .. 7 terms with one coefficient each (got {len(ks)}, {len(coeffs)})")
    for t in ks:
        if _chk(t, "k").numel() != n:
            raise ValueError(f"term has {t.numel()} elements, expected {n}")
    ptrs = (C.c_void_p * len(ks))(*[t.data_ptr() for t in ks])
    cf = (C.c_float * len(ks))(*[float(c) for c in coeffs])
    return C.cast(ptrs, C.c_void_p), C.cast(cf, C.c_void_p), (ptrs, cf)


def rk_combine(y0, ks, coeffs, out=None):
    """out = y0 + sum_j coeffs[j] * ks[j] (y0 may be None; at most 7 terms): the stage sums of an explicit Runge-Kutta step."""
    ref = ks[0]
    out = torch.empty_like(ref) if out is None else out
    kp, cp, keep = _rk_terms(ks, coeffs, ref.numel())
    if y0 is not None and _chk(y0, "y0").numel() != ref.numel():
        raise ValueError("rk_combine: y0 size")
    nat.check(nat.lib().kd_rk_combine_f32(_p(_chk(out, "out")), _p(y0), kp, cp, len(ks), ref.numel(), _stream()), "kd_rk_combine_f32")
    del keep
    return out


def rk_error_sq(ks, coeffs, y0, y1, atol, rtol):
    """sum over all elements of (sum_j coeffs[j] ks[j] / (atol + rtol * max(|y0|, |y1|)))^2 as a python float (one host sync): the square
    sum behind a Runge-Kutta error ratio.  y1 None: the scale is atol + rtol * |y0|."""
    return float(rk_error_partial(ks, coeffs, y0, y1, atol, rtol).double().sum().item())


def rk_error_partial(ks, coeffs, y0, y1, atol, rtol):
    """``rk_error_sq`` left on the device: its fixed grid of partial sums (fp32 [kd_rk_error_partials()]), for a caller that gathers
    several of them in one host read."""
    n = _chk(y0, "y0").numel()
    kp, cp, keep = _rk_terms(ks, coeffs, n)
    part = torch.empty(nat.lib().kd_rk_error_partials(), device=y0.device, dtype=torch.float32)
    nat.check(nat.lib().kd_rk_error_f32(kp, cp, len(ks), _p(y0), None if y1 is None else _p(_chk(y1, "y1")), float(atol), float(rtol), n, _p(part),
                                        _stream()), "kd_rk_error_f32")
    del keep
    return part


# ---- sample-quality metrics (csrc/metrics_f32.hip; evaluation.polynomial_kernel / squared_mmd / kid).  The Gram tiles follow the backward pass's
# rule (split3 unless exact); every sum runs in a fixed order through an fp64 workspace, so repeat calls give the same bits.

def _batch3(t, name):
    """[..., r, d] -> a contiguous [B, r, d] view and B."""
    _chk(t, name)
    r, d = t.shape[-2], t.shape[-1]
    b = t.numel() // max(1, r * d)
    return t.reshape(b, r, d), b


def _split3_of(x, precision):
    return (_prec_of(x) if precision is None else precision) != nat.PREC_EXACT


def mmd_poly(x, y, out=None, scale=1.0, accumulate=False, precision=None):
    """out[b] (+)= scale * squared MMD of x[b] [m, d] and y[b] [n, d] with the polynomial kernel (x . y / d + 1)^3, the kernel matrices never
    written.  x, y: [m, d] / [n, d] or [B, m, d] / [B, n, d]; out: [B] (or one element)."""
    x3, b = _batch3(x, "x")
    y3, by = _batch3(y, "y")
    m, d = x3.shape[1], x3.shape[2]
    n = y3.shape[1]
    if by != b or y3.shape[2] != d:
        raise ValueError(f"mmd_poly: x {tuple(x.shape)} and y {tuple(y.shape)} do not pair up")
    if out is None:
        if accumulate:
            raise ValueError("mmd_poly: accumulate needs out")
        out = torch.empty(b, device=x.device, dtype=torch.float32)
    elif _chk(out, "out").numel() != b:
        raise ValueError(f"mmd_poly: out has {out.numel()} elements for {b} batch items")
    tm, tn = -(-m // 64), -(-n // 64)
    ws = torch.empty(max(1, b * (tm * (tm + 1) // 2 + tn * (tn + 1) // 2 + tm * tn)), device=x.device, dtype=torch.float64)
    nat.check(nat.lib().kd_mmd_poly_f32(_p(x3), m * d, m, _p(y3), n * d, n, d, b, int(_split3_of(x, precision)), _p(ws), float(scale),
                                        int(bool(accumulate)), _p(out), _stream()), "kd_mmd_poly_f32")
    return out


def poly_kernel(x, y, precision=None):
    """(x y^T / d + 1)^3 of x [B, m, d] and y [B, n, d] (or [m, d] / [n, d]) -> [B, m, n] (or [m, n])."""
    x3, b = _batch3(x, "x")
    y3, by = _batch3(y, "y")
    m, d = x3.shape[1], x3.shape[2]
    n = y3.shape[1]
    if by != b or y3.shape[2] != d:
        raise ValueError(f"poly_kernel: x {tuple(x.shape)} and y {tuple(y.shape)} do not pair up")
    out = torch.empty(*x.shape[:-2], m, n, device=x.device, dtype=torch.float32)
    if out.numel():
        nat.check(nat.lib().kd_poly_kernel_f32(_p(x3), m * d, m, _p(y3), n * d, n, d, b, int(_split3_of(x, precision)), _p(out), _stream()),
                  "kd_poly_kernel_f32")
    return out


def mmd_mats(kxx, kyy, kxy):
    """Squared MMD from kernel matrices kxx [B, m, m], kyy [B, n, n], kxy [B, m, n] (diagonals of kxx and kyy dropped) -> [B]."""
    a, b = _batch3(kxx, "kxx")
    c, bc = _batch3(kyy, "kyy")
    e, be = _batch3(kxy, "kxy")
    m, n = a.shape[1], c.shape[1]
    if bc != b or be != b or a.shape[2] != m or c.shape[2] != n or e.shape[1:] != (m, n):
        raise ValueError(f"mmd_mats: kernel matrices {tuple(kxx.shape)}, {tuple(kyy.shape)}, {tuple(kxy.shape)} do not pair up")
    out = torch.empty(b, device=kxx.device, dtype=torch.float32)
    ws = torch.empty(max(1, b * 3 * (-(-max(m * m, n * n, m * n) // 4096))), device=kxx.device, dtype=torch.float64)
    nat.check(nat.lib().kd_mmd_mats_f32(_p(a), _p(c), _p(e), m, n, b, _p(ws), _p(out), _stream()), "kd_mmd_mats_f32")
    return out


# the eigensolver of sqrtm_eig / fid: one-sided Jacobi in fp64 (csrc/metrics_f32.hip), products of its factors on kd_gemm_tn_f64

JACOBI_MAX_SWEEPS = 60
jacobi_stats = {"sweeps": 0, "off": []}        # the last solve: its sweep count and the largest |cos| of each sweep (benchmarks read it)


def _f64(*shape, device):
    return torch.empty(*shape, device=device, dtype=torch.float64)


def jacobi_tol(n):
    """Rotation / convergence threshold on |cos| of two rows: a few fp64 ulps grown with sqrt(n), as in one-sided Jacobi SVD codes."""
    return 8.0 * math.sqrt(max(n, 1)) * 2.0 ** -52


def jacobi_rows(B, Vt=None):
    """One-sided Jacobi, in place, on the fp64 rows of B [batch, n, n] (and Vt, if given): afterwards the rows of B are mutually orthogonal,
    B = A V with row i of norm |lambda_i| (sigma_i), and Vt = V^T (when it started as I).  The convergence test reads one value per sweep."""
    b, n = B.shape[0], B.shape[-1]
    lib = nat.lib()
    conv, off = _f64(b * ((n + 1) // 2), device=B.device), _f64(1, device=B.device)
    tol, offs = jacobi_tol(n), []
    while len(offs) < JACOBI_MAX_SWEEPS:
        nat.check(lib.kd_jacobi_sweep_f64(_p(B), _p(Vt), b, n, tol, _p(conv), _p(off), _stream()), "kd_jacobi_sweep_f64")
        offs.append(off.item())
        if not offs[-1] > tol:
            break
    jacobi_stats.update(sweeps=len(offs), off=offs)
    return B, Vt


def sym_lower_f64(a, vectors=False, diag_add=0.0):
    """(B, Vt): the fp64 symmetric matrices of the lower triangles of a [batch, n, n] (fp32 or fp64) plus diag_add I, and Vt = I (if
    ``vectors``)."""
    b, n = a.shape[0], a.shape[-1]
    B = _f64(b, n, n, device=a.device)
    Vt = _f64(b, n, n, device=a.device) if vectors else None
    a64 = a.dtype == torch.float64
    nat.check(nat.lib().kd_sym_lower_f64(_p(_chk(a, "a", a.dtype if a64 else torch.float32)), int(a64), _p(B), _p(Vt), b, n, float(diag_add),
                                         _stream()), "kd_sym_lower_f64")
    return B, Vt


def row_sqrt_norm_f64(B):
    """sqrt(||row||) of every row of B [batch, n, n] -> [batch, n] (fp64)."""
    n = B.shape[-1]
    out = _f64(*B.shape[:-1], device=B.device)
    nat.check(nat.lib().kd_row_sqrt_norm_f64(_p(_chk(B, "B", torch.float64)), B.numel() // n, n, _p(out), _stream()), "kd_row_sqrt_norm_f64")
    return out


def gemm_tn_f64(G, A, row_scale=None, out32=False):
    """G[b]^T diag(row_scale[b]) A[b] in fp64 for G [batch, M, N], A [batch, M, K] -> [batch, N, K] (fp64, or rounded to fp32)."""
    b, M, N = G.shape
    K = A.shape[-1]
    if A.shape[:2] != (b, M) or (row_scale is not None and row_scale.shape != (b, M)):
        raise ValueError(f"gemm_tn_f64: G {tuple(G.shape)}, A {tuple(A.shape)} do not pair up")
    out = torch.empty(b, N, K, device=G.device, dtype=torch.float32 if out32 else torch.float64)
    nat.check(nat.lib().kd_gemm_tn_f64(_p(_chk(G, "G", torch.float64)), _p(_chk(A, "A", torch.float64)),
                                       _p(None if row_scale is None else _chk(row_scale, "row_scale", torch.float64)), b, M, N, K,
                                       None if out32 else _p(out), _p(out) if out32 else None, _stream()), "kd_gemm_tn_f64")
    return out


def center(x):
    """(x - mean in fp64, mean) of x [rows, d] over its rows; the column sums from ``colsum``."""
    rows, d = x.shape
    s = colsum(x)
    xc = _f64(rows, d, device=x.device)
    mean = torch.empty(d, device=x.device, dtype=torch.float32)
    nat.check(nat.lib().kd_center_f32(_p(_chk(x, "x")), _p(s), rows, d, _p(xc), _p(mean), _stream()), "kd_center_f32")
    return xc, mean


def transpose_f64(a):
    """a[b]^T for a [batch, n, n] (fp64)."""
    out = torch.empty_like(a)
    nat.check(nat.lib().kd_transpose_f64(_p(_chk(a, "a", torch.float64)), _p(out), a.shape[0], a.shape[-1], _stream()), "kd_transpose_f64")
    return out


def sqrtm_vjp_div_f64(m, s):
    """m[b, i, j] / (s[b, i] + s[b, j]) for m [batch, n, n], s [batch, n] (fp64)."""
    out = torch.empty_like(m)
    nat.check(nat.lib().kd_sqrtm_vjp_div_f64(_p(_chk(m, "m", torch.float64)), _p(_chk(s, "s", torch.float64)), m.shape[0], m.shape[-1], _p(out),
                                             _stream()), "kd_sqrtm_vjp_div_f64")
    return out


def to_f64(a):
    out = torch.empty(a.shape, device=a.device, dtype=torch.float64)
    if a.numel():
        nat.check(nat.lib().kd_f32_to_f64(_p(_chk(a, "a")), _p(out), a.numel(), _stream()), "kd_f32_to_f64")
    return out


def fid_finish(mean_x, mean_y, cov_x, cov_y, sq):
    """|mean_x - mean_y|^2 + tr cov_x + tr cov_y - 2 sum(sq) -> a 0-dim fp32 tensor (fp64 covariances and sums)."""
    d = mean_x.numel()
    out = torch.empty((), device=mean_x.device, dtype=torch.float32)
    nat.check(nat.lib().kd_fid_finish_f32(_p(_chk(mean_x, "mean_x")), _p(_chk(mean_y, "mean_y")), _p(_chk(cov_x, "cov_x", torch.float64)),
                                          _p(_chk(cov_y, "cov_y", torch.float64)), _p(_chk(sq, "sq", torch.float64)), d, _p(out), _stream()),
              "kd_fid_finish_f32")
    return out


def sigma_density(kind, u, params, normal=None, group=0, groups=0, dtype=None):
    """sigmas from uniform draws ``u`` (fp32 or fp64, any shape) under density ``kind`` (nat.DENSITY_*) with up to 8 host constants
    ``params`` (include/kdiff_hip.h: kd_sigma_density_f32); ``normal``: standard normal draws of u's shape and dtype for the split
    log-normal.  ``groups > 0`` folds the stratification of utils.stratified_uniform over u's last dimension in.  Output fp32, or fp64
    with ``dtype=torch.float64``."""
    _chk(u, "u", u.dtype if isinstance(u, torch.Tensor) and u.dtype == torch.float64 else torch.float32)
    if normal is not None:
        _chk(normal, "normal", u.dtype)
        if normal.shape != u.shape:
            raise ValueError("sigma_density: normal and u differ in shape")
    out = torch.empty(u.shape, device=u.device, dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    if u.numel():
        prm = (C.c_double * 8)(*[float(v) for v in params], *([0.0] * (8 - len(params))))
        nat.check(nat.lib().kd_sigma_density_f32(int(kind), _p(u), int(u.dtype == torch.float64), _p(normal), _p(out),
                                                 int(out.dtype == torch.float64), u.numel(), u.shape[-1] if u.ndim else 1, int(group), int(groups),
                                                 prm, _stream()), "kd_sigma_density_f32")
    return out

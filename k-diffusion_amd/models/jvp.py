"""Dual pass (forward-mode JVP) of the hourglass transformer: ``ImageTransformerDenoiserModelV2.forward_jvp``.

One call runs the network's primal x and a tangent x_dot side by side and returns (F(x), J_F(x) x_dot) -- or, with ``sigma_data``, the
same for the Karras denoiser D(x) = F(x c_in) c_out + x c_skip.  It is what ``log_likelihood`` needs for its divergence term v^T (J v)
(k_diffusion/sampling.py:287-293 takes v . (v^T J) in reverse mode instead; the two are the same number).

Composition, level by level as the model (image_transformer_v2.py:721-762), from unfused ``ops`` calls:
  - the conditioning (sigma -> mapping network -> AdaRMSNorm scales) has a zero tangent: its scales are computed once per call;
  - every linear piece -- patch-in (with c_in: linear in x), the qkv / out / up / down projections, token merge, TokenSplit + lerp,
    the residual adds, patch-out (with c_out F + c_skip x) -- runs its tangent through the same GEMM as the primal;
  - the nonlinear pieces have HIP rules of their own (csrc/jvp_f32.hip): RMSNorm / AdaRMSNorm, GEGLU, the cosine-sim scale + RoPE of
    q, k, and the three attention geometries.
Patch-out runs as the RMSNorm rule with the shared ``out_norm`` gain, then the un-normalised un-patch GEMM.

Arithmetic: fp32 activations in every KDIFF_GEMM mode -- their GEMMs run split3 under ``split3`` / ``bf16`` / ``fp8`` (ops._prec_of) and
exact fp32 under ``exact``; the rules above are fp32 FMAs.  The primal half therefore agrees with ``forward`` to the split3 tolerance, not
bit for bit (``forward`` runs the fused kernels of its launch plan).  The dual pass builds, reads and evicts no launch plan.
"""
import torch

from .. import ops
from . import axial_rope

EPS = 1e-6


def _rope(model, li, grids, sa, device):
    """cos / sin tables of a layer's AxialRoPE at level ``li`` (kept per model, keyed by the frequencies tensor and the grid)."""
    cache = model.__dict__.setdefault("_jvp_rope", {})
    freqs = sa.pos_emb.freqs
    key = (id(freqs), freqs._version if not freqs.is_inference() else None, li, tuple(grids[0]), device)
    ent = cache.get(key)
    if ent is None or ent[0] is not freqs:
        if len(cache) > 256:
            cache.clear()
        h0, w0 = grids[0]
        pos = axial_rope.make_axial_pos(h0, w0).view(h0, w0, 2)
        for _ in range(li):
            pos = axial_rope.downscale_pos(pos)
        cos_t, sin_t = axial_rope.rope_tables(pos, freqs.detach().cpu())
        ent = cache[key] = (freqs, cos_t.to(device).contiguous(), sin_t.to(device).contiguous())
    return ent[1], ent[2]


def _conditioning(model, sigma, aug_cond, class_cond, mapping_cond):
    """The mapping network's output [B, mapping width] (image_transformer_v2.py:729-740, :552-581) on ``ops`` calls."""
    m = model
    B = sigma.shape[0]
    dev = sigma.device
    ff = ops.fourier_sigma(sigma, m.time_emb.weight.detach().contiguous())
    temb = ops.linear(ff, m.time_in_proj.weight)
    aug = torch.zeros(B, 9, device=dev, dtype=torch.float32) if aug_cond is None else aug_cond.to(device=dev, dtype=torch.float32).reshape(B, 9).contiguous()
    aug_proj = ops.linear(ops.fourier_features(aug, m.aug_emb.weight.detach().contiguous()), m.aug_in_proj.weight)
    emb = ids = None
    if m.class_emb is not None:
        ids = class_cond.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
        lo, hi = (int(ids.min()), int(ids.max()))
        if lo < 0 or hi >= m.class_emb.weight.shape[0]:
            raise IndexError(f"class_cond ids must lie in [0, {m.class_emb.weight.shape[0] - 1}] (got {lo}..{hi})")
        emb = m.class_emb.weight
    mterm = None
    if m.mapping_cond_in_proj is not None:
        mterm = ops.linear(mapping_cond.to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous(), m.mapping_cond_in_proj.weight)
    c = ops.cond_sum(temb, aug_proj, emb=emb, ids=ids, c=mterm)
    c = ops.rms_norm(c, m.mapping.in_norm.scale)
    for blk in m.mapping.blocks:
        h = ops.norm_linear(c, blk.norm.scale, blk.up_proj.weight, rows_per_sample=B, epi=ops.nat.EPI_GEGLU)
        c = ops.linear(h, blk.down_proj.weight, residual=c)
    return ops.rms_norm(c, m.mapping.out_norm.scale)


def _ada_scale(cond, norm):
    """AdaRMSNorm scales (:155-166): Linear(cond) + 1 -> [B, d]."""
    return ops.linear(cond, norm.linear.weight, out_add=1.0)


def _layer(model, li, mod, index, grids, x, xd, cond):
    lv = model.level_specs[li]
    spec = lv.self_attn
    B, gh, gw, d = x.shape
    rps = gh * gw
    if hasattr(mod, "self_attn"):
        sa = mod.self_attn
        nh = d // spec.d_head
        h, hd = ops.rms_norm_jvp(x, xd, _ada_scale(cond, sa.norm), rows_per_sample=rps)
        qkv, qkvd = ops.linear(h, sa.qkv_proj.weight), ops.linear(hd, sa.qkv_proj.weight)
        cos_t, sin_t = _rope(model, li, grids, sa, x.device)
        ops.qk_prep_jvp_(qkv, qkvd, sa.scale.detach().contiguous(), cos_t, sin_t, nh, EPS)
        kind = type(spec).__name__
        if kind == "GlobalAttentionSpec":
            o, od = ops.attn_global_jvp(qkv, qkvd, nh)
        elif kind == "NeighborhoodAttentionSpec":
            o, od = ops.attn_na2d_jvp(qkv, qkvd, nh, spec.kernel_size)
        else:
            ws = spec.window_size
            o, od = ops.attn_window_jvp(qkv, qkvd, nh, ws, ws // 2 if index % 2 == 1 else 0)      # shift: :523
        x, xd = ops.linear(o, sa.out_proj.weight, residual=x), ops.linear(od, sa.out_proj.weight, residual=xd)
    ff = mod.ff
    h, hd = ops.rms_norm_jvp(x, xd, _ada_scale(cond, ff.norm), rows_per_sample=rps)
    u, ud = ops.linear(h, ff.up_proj.weight), ops.linear(hd, ff.up_proj.weight)        # [value | gate] rows (linear_geglu, :89-95)
    g, gd = ops.geglu_jvp(u, ud)
    return ops.linear(g, ff.down_proj.weight, residual=x), ops.linear(gd, ff.down_proj.weight, residual=xd)


@torch.no_grad()
def forward_jvp(model, x, sigma, x_dot, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None):
    """(out, out_dot) of the inner model F (``sigma_data`` None) or of the Karras denoiser around it (``sigma_data`` given)."""
    m = model
    if class_cond is None and m.class_emb is not None:
        raise ValueError("class_cond must be specified if num_classes > 0")
    if mapping_cond is None and m.mapping_cond_in_proj is not None:
        raise ValueError("mapping_cond must be specified if mapping_cond_dim > 0")
    if x.dim() != 4 or x.shape[1] != m.in_channels:
        raise ValueError(f"expected input [B, {m.in_channels}, H, W], got {tuple(x.shape)}")
    if x_dot.shape != x.shape:
        raise ValueError(f"tangent shape {tuple(x_dot.shape)} != input shape {tuple(x.shape)}")
    if not x.is_cuda or not x_dot.is_cuda:
        raise RuntimeError("forward_jvp runs on the HIP path only: move the model and inputs to a ROCm device (there is no CPU fallback)")
    if x.dtype != torch.float32 or x_dot.dtype != torch.float32:
        raise TypeError(f"fp32 inputs only (got {x.dtype}, {x_dot.dtype})")
    if m.patch_in.proj.weight.device != x.device:
        raise RuntimeError(f"model weights are on {m.patch_in.proj.weight.device}, input on {x.device}")
    x, x_dot = x.contiguous(), x_dot.contiguous()
    B, _, H, W = x.shape
    ph, pw = m.patch_size
    if H % ph or W % pw:
        raise ValueError(f"input {H}x{W} not divisible by the patch size {ph}x{pw}")
    levels = m.level_specs
    grids = [(H // ph, W // pw)]
    for _ in range(len(levels) - 1):
        gh, gw = grids[-1]
        if gh % 2 or gw % 2:
            raise ValueError(f"token grid {gh}x{gw} cannot be merged 2x2")
        grids.append((gh // 2, gw // 2))
    sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    prec = ops._prec_of(x)
    pre = dict(sigma=sigma, sigma_data=float(sigma_data)) if sigma_data is not None else {}
    cond = _conditioning(m, sigma, aug_cond, class_cond, mapping_cond)

    h = ops.patch_in(x, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    hd = ops.patch_in(x_dot, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    skips = []
    n_lv = len(levels)
    for li in range(n_lv - 1):
        for i, mod in enumerate(m.down_levels[li]):
            h, hd = _layer(m, li, mod, i, grids, h, hd, cond)
        skips.append((h, hd))
        w = m.merges[li].proj.weight
        h, hd = ops.token_merge(h, w), ops.token_merge(hd, w)
    for i, mod in enumerate(m.mid_level):
        h, hd = _layer(m, n_lv - 1, mod, i, grids, h, hd, cond)
    for li in reversed(range(n_lv - 1)):
        sp, (s, sd) = m.splits[li], skips[li]
        fac = sp.fac.detach().contiguous()
        h, hd = ops.token_split_lerp(h, sp.proj.weight, s, fac), ops.token_split_lerp(hd, sp.proj.weight, sd, fac)
        for i, mod in enumerate(m.up_levels[li]):
            h, hd = _layer(m, li, mod, i + levels[li].depth, grids, h, hd, cond)        # :697
    h, hd = ops.rms_norm_jvp(h, hd, m.out_norm.scale.detach().contiguous())
    w = m.patch_out.proj.weight
    skip, skip_d = (x, x_dot) if sigma_data is not None else (None, None)
    out = ops.patch_out(h, None, w, m.patch_size, m.out_channels, x_in=skip, **pre)
    out_d = ops.patch_out(hd, None, w, m.patch_size, m.out_channels, x_in=skip_d, **pre)
    return out, out_d

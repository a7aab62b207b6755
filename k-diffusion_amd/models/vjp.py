"""Backward pass (reverse-mode VJP) of the hourglass transformer w.r.t. its input: what autograd calls for ``ImageTransformerDenoiserModelV2``.

``backward(model, x, sigma, grad_out, ...)`` returns J^T grad_out for the inner model F (``sigma_data`` None) or for the Karras denoiser
D(x) = F(x c_in) c_out + x c_skip (``sigma_data`` given).  Gradient guidance (a loss on the denoised image differentiated w.r.t. x on every
solver step) and the reference's autograd form of log_likelihood (k_diffusion/sampling.py:286-294) need it.  The conditioning and the
weights are held fixed: sigma, aug_cond, class_cond, mapping_cond and the parameters get no gradient (training is out of scope).

Recompute, do not save: autograd keeps only the inputs.  The backward pass reruns the primal on the unfused fp32 ``ops`` path keeping one
tensor per layer input (and per skip), then walks the network in reverse, level by level as ``jvp.py`` walks it forward, recomputing inside
each layer (its norm, qkv, q/k preparation and the attention statistics) as it gets there.
  - every linear piece runs its transpose on the existing GEMMs with transposed weights (built once per model, ``_wt``): the projections;
    TokenMerge^T as the depth-to-space scatter of TokenSplit's epilogue (lerp weight 1); TokenSplit + lerp^T as the 2x2 gather of TokenMerge
    with fac W^T, its skip taking (1 - fac) of the gradient; patch-in^T as the un-patch epilogue, patch-out^T as the patch gather, with the
    preconditioning's per-sample c_in / c_out / c_skip on ``ops.precond_vjp``; the residual adds pass the gradient through.
  - the nonlinear pieces have HIP rules of their own (csrc/vjp_f32.hip): RMSNorm / AdaRMSNorm, GEGLU, the cosine-sim scale + RoPE of q, k, and
    the three attention geometries (flash-attention-2's query and key sweeps; the neighbourhood's key sweep runs over its inverse window).
Arithmetic: fp32 in every KDIFF_GEMM mode, as the dual pass (split3 GEMMs under ``split3`` / ``bf16`` / ``fp8``, exact fp32 under
``exact``).  No launch plan is built, read or evicted.
"""
import torch

from .. import ops
from . import jvp

EPS = jvp.EPS


def _wt(model, w, fac=None):
    """W^T (or (fac W)^T) of a weight as a contiguous tensor, kept per model: keyed by the tensor objects and their version counters, so an
    in-place update of the weight (or of fac) builds it again."""
    cache = model.__dict__.setdefault("_vjp_wt", {})
    ver = lambda t: None if t is None else (id(t), t._version if not t.is_inference() else None)
    key = (ver(w), ver(fac), w.device)
    ent = cache.get(key)
    if ent is None or ent[0] is not w or ent[1] is not fac:
        if len(cache) > 512:
            cache.clear()
        t = w.detach() if fac is None else w.detach() * fac.detach()
        ent = cache[key] = (w, fac, t.t().contiguous())
    return ent[2]


def _split_consts(model, sp, B, device):
    """(1 - fac) and 1 per sample (rows of ``ops.rows_affine``) and the lerp weight 1 of the depth-to-space scatter, kept per model."""
    cache = model.__dict__.setdefault("_vjp_split", {})
    fac = sp.fac
    key = (id(fac), fac._version if not fac.is_inference() else None, B, device)
    ent = cache.get(key)
    if ent is None or ent[0] is not fac:
        if len(cache) > 256:
            cache.clear()
        f = fac.detach().to(device=device, dtype=torch.float32).reshape(1)
        ent = cache[key] = (fac, (1 - f).expand(B).contiguous(), torch.ones(B, device=device), torch.ones(1, device=device))
    return ent[1:]


def _attn_fwd(model, li, mod, index, grids, x, cond, keep):
    """The self-attention sublayer (:466-476) from its input x: returns x + out_proj(attn), and with ``keep`` what its reverse needs (the
    AdaRMSNorm scale, the unprepared and the prepared qkv, the RoPE tables)."""
    spec = model.level_specs[li].self_attn
    sa = mod.self_attn
    B, gh, gw, d = x.shape
    nh = d // spec.d_head
    s = jvp._ada_scale(cond, sa.norm)
    qkv = ops.norm_linear(x, s, sa.qkv_proj.weight, rows_per_sample=gh * gw)
    prep = qkv.clone() if keep else qkv
    cos_t, sin_t = jvp._rope(model, li, grids, sa, x.device)
    ops.qk_prep_(prep, sa.scale.detach().contiguous(), cos_t, sin_t, nh, EPS)
    kind = type(spec).__name__
    if kind == "GlobalAttentionSpec":
        o = ops.attn_global(prep, nh)
    elif kind == "NeighborhoodAttentionSpec":
        o = ops.attn_na2d(prep, nh, spec.kernel_size)
    else:
        ws = spec.window_size
        o = ops.attn_window(prep, nh, ws, ws // 2 if index % 2 == 1 else 0)      # shift: :523
    x = ops.linear(o, sa.out_proj.weight, residual=x)
    return x, ((s, qkv, prep, cos_t, sin_t) if keep else None)


def _layer_fwd(model, li, mod, index, grids, x, cond):
    if hasattr(mod, "self_attn"):
        x, _ = _attn_fwd(model, li, mod, index, grids, x, cond, keep=False)
    ff = mod.ff
    rps = x.shape[1] * x.shape[2]
    h = ops.norm_linear(x, jvp._ada_scale(cond, ff.norm), ff.up_proj.weight, rows_per_sample=rps, epi=ops.nat.EPI_GEGLU)
    return ops.linear(h, ff.down_proj.weight, residual=x)


def _layer_vjp(model, li, mod, index, grids, x, g, cond):
    """Gradient w.r.t. a layer's input x from the gradient g on its output; the layer's insides are recomputed from x."""
    B, gh, gw, d = x.shape
    rps = gh * gw
    has_attn = hasattr(mod, "self_attn")
    if has_attn:
        xf, (s_a, qkv, prep, cos_t, sin_t) = _attn_fwd(model, li, mod, index, grids, x, cond, keep=True)
    else:
        xf = x
    ff = mod.ff
    s_f = jvp._ada_scale(cond, ff.norm)
    u = ops.norm_linear(xf, s_f, ff.up_proj.weight, rows_per_sample=rps)           # [value | gate] rows (linear_geglu, :89-95)
    gu = ops.geglu_vjp(u, ops.linear(g, _wt(model, ff.down_proj.weight)))
    g = ops.rms_norm_vjp(xf, ops.linear(gu, _wt(model, ff.up_proj.weight)), s_f, rows_per_sample=rps, add=g)
    if not has_attn:
        return g
    sa = mod.self_attn
    spec = model.level_specs[li].self_attn
    nh = d // spec.d_head
    go = ops.linear(g, _wt(model, sa.out_proj.weight))
    kind = type(spec).__name__
    if kind == "GlobalAttentionSpec":
        gq = ops.attn_global_vjp(prep, go, nh)
    elif kind == "NeighborhoodAttentionSpec":
        gq = ops.attn_na2d_vjp(prep, go, nh, spec.kernel_size)
    else:
        ws = spec.window_size
        gq = ops.attn_window_vjp(prep, go, nh, ws, ws // 2 if index % 2 == 1 else 0)
    ops.qk_prep_vjp_(qkv, gq, sa.scale.detach().contiguous(), cos_t, sin_t, nh, EPS)
    return ops.rms_norm_vjp(x, ops.linear(gq, _wt(model, sa.qkv_proj.weight)), s_a, rows_per_sample=rps, add=g)


@torch.no_grad()
def backward(model, x, sigma, grad_out, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None):
    """J^T grad_out w.r.t. x of the inner model F (``sigma_data`` None) or of the Karras denoiser around it (``sigma_data`` given)."""
    m = model
    if class_cond is None and m.class_emb is not None:
        raise ValueError("class_cond must be specified if num_classes > 0")
    if mapping_cond is None and m.mapping_cond_in_proj is not None:
        raise ValueError("mapping_cond must be specified if mapping_cond_dim > 0")
    if x.dim() != 4 or x.shape[1] != m.in_channels:
        raise ValueError(f"expected input [B, {m.in_channels}, H, W], got {tuple(x.shape)}")
    if not x.is_cuda or not grad_out.is_cuda:
        raise RuntimeError("the backward pass runs on the HIP path only: move the model and inputs to a ROCm device (there is no CPU fallback)")
    if x.dtype != torch.float32 or grad_out.dtype != torch.float32:
        raise TypeError(f"fp32 inputs only (got {x.dtype}, {grad_out.dtype})")
    B, _, H, W = x.shape
    if grad_out.shape != (B, m.out_channels, H, W):
        raise ValueError(f"gradient shape {tuple(grad_out.shape)} != output shape {(B, m.out_channels, H, W)}")
    if m.patch_in.proj.weight.device != x.device:
        raise RuntimeError(f"model weights are on {m.patch_in.proj.weight.device}, input on {x.device}")
    x, grad_out = x.contiguous(), grad_out.contiguous()
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
    cond = jvp._conditioning(m, sigma, aug_cond, class_cond, mapping_cond)

    # primal, keeping every layer's input (image_transformer_v2.py:721-762)
    acts, skips = [], []
    n_lv = len(levels)
    h = ops.patch_in(x, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    for li in range(n_lv - 1):
        for i, mod in enumerate(m.down_levels[li]):
            acts.append((li, mod, i, h))
            h = _layer_fwd(m, li, mod, i, grids, h, cond)
        skips.append(h)
        h = ops.token_merge(h, m.merges[li].proj.weight)
    for i, mod in enumerate(m.mid_level):
        acts.append((n_lv - 1, mod, i, h))
        h = _layer_fwd(m, n_lv - 1, mod, i, grids, h, cond)
    for li in reversed(range(n_lv - 1)):
        sp = m.splits[li]
        h = ops.token_split_lerp(h, sp.proj.weight, skips[li], sp.fac.detach().contiguous())
        for i, mod in enumerate(m.up_levels[li]):
            acts.append((li, mod, i + levels[li].depth, h))                       # :697
            h = _layer_fwd(m, li, mod, i + levels[li].depth, grids, h, cond)
    del skips

    # reverse walk
    g_img = ops.precond_vjp(grad_out, ops.nat.PC_OUT, sigma, sigma_data) if sigma_data is not None else grad_out
    g = ops.patch_in(g_img, _wt(m, m.patch_out.proj.weight), m.patch_size, precision=prec)     # patch-out^T: the patch gather
    g = ops.rms_norm_vjp(h, g, m.out_norm.scale.detach().contiguous())
    del h
    g_split = []
    for li in range(n_lv - 1):
        for _ in m.up_levels[li]:
            g = _pop_vjp(m, acts, grids, g, cond)
        sp = m.splits[li]
        g_split.append(g)                                                          # the skip's share: (1 - fac) g, taken at the merge
        g = ops.token_merge(g, _wt(m, sp.proj.weight, fac=sp.fac))
    for _ in m.mid_level:
        g = _pop_vjp(m, acts, grids, g, cond)
    for li in reversed(range(n_lv - 1)):
        omf, ones, one = _split_consts(m, m.splits[li], B, x.device)
        gs = g_split[li]
        g = ops.token_split_lerp(g, _wt(m, m.merges[li].proj.weight), gs, one)     # TokenMerge^T: depth-to-space (lerp weight 1)
        g = ops.rows_affine(gs, omf, g, ones)
        for _ in m.down_levels[li]:
            g = _pop_vjp(m, acts, grids, g, cond)
    g = ops.patch_out(g, None, _wt(m, m.patch_in.proj.weight), m.patch_size, m.in_channels)   # patch-in^T: the un-patch
    if sigma_data is not None:
        g = ops.precond_vjp(g, ops.nat.PC_IN, sigma, sigma_data, h=grad_out, h_coef=ops.nat.PC_SKIP)
    return g


def _pop_vjp(model, acts, grids, g, cond):
    li, mod, index, x = acts.pop()
    return _layer_vjp(model, li, mod, index, grids, x, g, cond)

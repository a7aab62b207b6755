"""Backward pass (reverse-mode VJP) of the hourglass transformer w.r.t. its input: what autograd calls for ``ImageTransformerDenoiserModelV2``.

``backward(model, x, sigma, grad_out, ...)`` returns J^T grad_out for the inner model F (``sigma_data`` None) or for the Karras denoiser
D(x) = F(x c_in) c_out + x c_skip (``sigma_data`` given).  Gradient guidance (a loss on the denoised image differentiated w.r.t. x on every
solver step) and the reference's autograd form of log_likelihood (k_diffusion/sampling.py:286-294) need it.  The conditioning and the
weights are held fixed: sigma, aug_cond, class_cond, mapping_cond and the parameters get no gradient (training is out of scope).

Recompute, do not save: autograd keeps only the inputs.  The backward pass reruns the primal on the unfused fp32 ``ops`` path keeping one
tensor per layer input (and per skip), then walks the model's steps (``image_transformer_v2.hourglass``) in reverse, recomputing inside each
layer (its norm, qkv, q/k preparation and the attention statistics) as it gets there.
  - every linear piece runs its transpose on the existing GEMMs with transposed weights (``_wt``: kept in the model's store of
    weight-derived tensors, ``_derive``): the projections;
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
from . import image_transformer_v2 as itv2


def _wt(model, w, fac=None):
    """W^T (or (fac W)^T) of a weight as a contiguous tensor, kept per model (``_derive``: an in-place update of w or fac builds it
    again)."""
    if fac is None:
        return model._derive(("wt", w.device), (w,), lambda: w.detach().t().contiguous())
    return model._derive(("wt", w.device), (w, fac), lambda: (w.detach() * fac.detach()).t().contiguous())


def _split_consts(model, sp, B, device):
    """(1 - fac) and 1 per sample (rows of ``ops.rows_affine``) and the lerp weight 1 of the depth-to-space scatter, kept per model."""
    def build():
        f = sp.fac.detach().to(device=device, dtype=torch.float32).reshape(1)
        return (1 - f).expand(B).contiguous(), torch.ones(B, device=device), torch.ones(1, device=device)
    return model._derive(("split", B, device), (sp.fac,), build)


def _attn_fwd(model, st, grids, x, cond, keep):
    """The self-attention sublayer (:466-476) of layer step ``st`` from its input x: returns x + out_proj(attn), and with ``keep`` what
    its reverse needs (the AdaRMSNorm scale, the unprepared and the prepared qkv, the RoPE tables)."""
    spec = model.level_specs[st.level].self_attn
    sa = st.module.self_attn
    B, gh, gw, d = x.shape
    nh = d // spec.d_head
    s = itv2.ada_scale(cond, sa.norm)
    qkv = ops.norm_linear(x, s, sa.qkv_proj.weight, rows_per_sample=gh * gw)
    prep = qkv.clone() if keep else qkv
    cos_t, sin_t = model._rope(st.level, grids, sa, x.device)
    ops.qk_prep_(prep, sa.scale.detach().contiguous(), cos_t, sin_t, nh, itv2.EPS)
    _, core, params = itv2.attn_geometry(spec, st.index)
    o = getattr(ops, core)(prep, nh, *params)
    x = ops.linear(o, sa.out_proj.weight, residual=x)
    return x, ((s, qkv, prep, cos_t, sin_t) if keep else None)


def _layer_fwd(model, st, grids, x, cond):
    if hasattr(st.module, "self_attn"):
        x, _ = _attn_fwd(model, st, grids, x, cond, keep=False)
    ff = st.module.ff
    rps = x.shape[1] * x.shape[2]
    h = ops.norm_linear(x, itv2.ada_scale(cond, ff.norm), ff.up_proj.weight, rows_per_sample=rps, epi=ops.nat.EPI_GEGLU)
    return ops.linear(h, ff.down_proj.weight, residual=x)


def _layer_vjp(model, st, grids, x, g, cond):
    """Gradient w.r.t. the input x of layer step ``st`` from the gradient g on its output; the layer's insides are recomputed from x."""
    B, gh, gw, d = x.shape
    rps = gh * gw
    has_attn = hasattr(st.module, "self_attn")
    if has_attn:
        xf, (s_a, qkv, prep, cos_t, sin_t) = _attn_fwd(model, st, grids, x, cond, keep=True)
    else:
        xf = x
    ff = st.module.ff
    s_f = itv2.ada_scale(cond, ff.norm)
    u = ops.norm_linear(xf, s_f, ff.up_proj.weight, rows_per_sample=rps)           # [value | gate] rows (linear_geglu, :89-95)
    gu = ops.geglu_vjp(u, ops.linear(g, _wt(model, ff.down_proj.weight)))
    g = ops.rms_norm_vjp(xf, ops.linear(gu, _wt(model, ff.up_proj.weight)), s_f, rows_per_sample=rps, add=g)
    if not has_attn:
        return g
    sa = st.module.self_attn
    spec = model.level_specs[st.level].self_attn
    nh = d // spec.d_head
    go = ops.linear(g, _wt(model, sa.out_proj.weight))
    _, core, params = itv2.attn_geometry(spec, st.index)
    gq = getattr(ops, core + "_vjp")(prep, go, nh, *params)
    ops.qk_prep_vjp_(qkv, gq, sa.scale.detach().contiguous(), cos_t, sin_t, nh, itv2.EPS)
    return ops.rms_norm_vjp(x, ops.linear(gq, _wt(model, sa.qkv_proj.weight)), s_a, rows_per_sample=rps, add=g)


@torch.no_grad()
def backward(model, x, sigma, grad_out, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None):
    """J^T grad_out w.r.t. x of the inner model F (``sigma_data`` None) or of the Karras denoiser around it (``sigma_data`` given)."""
    m = model
    x, grad_out = m._check_input(x, class_cond, mapping_cond, "the backward pass",
                                 (grad_out, m.out_channels, "gradient shape {} != output shape {}"))
    grids = m._token_grids(x)
    B = x.shape[0]
    sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    prec = ops._prec_of(x)
    pre = dict(sigma=sigma, sigma_data=float(sigma_data)) if sigma_data is not None else {}
    cond = itv2.conditioning(m, sigma, aug_cond, class_cond, mapping_cond)
    steps = itv2.hourglass(m)

    # primal, keeping every layer's input (image_transformer_v2.py:721-762)
    acts, skips = [], []
    h = ops.patch_in(x, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    for st in steps:
        if st.kind == "layer":
            acts.append(h)
            h = _layer_fwd(m, st, grids, h, cond)
        elif st.kind == "merge":
            skips.append(h)
            h = ops.token_merge(h, m.merges[st.level].proj.weight)
        else:
            sp = m.splits[st.level]
            h = ops.token_split_lerp(h, sp.proj.weight, skips.pop(), sp.fac.detach().contiguous())

    # reverse walk
    g_img = ops.precond_vjp(grad_out, ops.nat.PC_OUT, sigma, sigma_data) if sigma_data is not None else grad_out
    g = ops.patch_in(g_img, _wt(m, m.patch_out.proj.weight), m.patch_size, precision=prec)     # patch-out^T: the patch gather
    g = ops.rms_norm_vjp(h, g, m.out_norm.scale.detach().contiguous())
    del h
    g_skips = []
    for st in reversed(steps):
        if st.kind == "layer":
            g = _layer_vjp(m, st, grids, acts.pop(), g, cond)
        elif st.kind == "split":
            sp = m.splits[st.level]
            g_skips.append(g)                                                          # the skip's share: (1 - fac) g, taken at the merge
            g = ops.token_merge(g, _wt(m, sp.proj.weight, fac=sp.fac))
        else:
            omf, ones, one = _split_consts(m, m.splits[st.level], B, x.device)
            gs = g_skips.pop()
            g = ops.token_split_lerp(g, _wt(m, m.merges[st.level].proj.weight), gs, one)     # TokenMerge^T: depth-to-space (lerp weight 1)
            g = ops.rows_affine(gs, omf, g, ones)
    g = ops.patch_out(g, None, _wt(m, m.patch_in.proj.weight), m.patch_size, m.in_channels)   # patch-in^T: the un-patch
    if sigma_data is not None:
        g = ops.precond_vjp(g, ops.nat.PC_IN, sigma, sigma_data, h=grad_out, h_coef=ops.nat.PC_SKIP)
    return g

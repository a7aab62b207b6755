"""Dual pass (forward-mode JVP) of the hourglass transformer: ``ImageTransformerDenoiserModelV2.forward_jvp``.

One call runs the network's primal x and a tangent x_dot side by side and returns (F(x), J_F(x) x_dot) -- or, with ``sigma_data``, the
same for the Karras denoiser D(x) = F(x c_in) c_out + x c_skip.  It is what ``log_likelihood`` needs for its divergence term v^T (J v)
(k_diffusion/sampling.py:287-293 takes v . (v^T J) in reverse mode instead; the two are the same number).

Composition, step by step along the model's walk (``image_transformer_v2.hourglass``), from unfused ``ops`` calls:
  - the conditioning (sigma -> mapping network -> AdaRMSNorm scales, ``image_transformer_v2.conditioning``) has a zero tangent: its
    scales are computed once per call;
  - every linear piece -- patch-in (with c_in: linear in x), the qkv / out / up / down projections, token merge, TokenSplit + lerp,
    the residual adds, patch-out (with c_out F + c_skip x) -- runs its tangent through the same GEMM as the primal;
  - the nonlinear pieces have HIP rules of their own (csrc/jvp_f32.hip): RMSNorm / AdaRMSNorm, GEGLU, the cosine-sim scale + RoPE of
    q, k (RoPE tables from the model's store of weight-derived tensors, ``_rope``), and the three attention geometries
    (``image_transformer_v2.attn_geometry`` picks ops.<core>_jvp).
Patch-out runs as the RMSNorm rule with the shared ``out_norm`` gain, then the un-normalised un-patch GEMM.

Arithmetic: fp32 activations in every KDIFF_GEMM mode -- their GEMMs run split3 under ``split3`` / ``bf16`` / ``fp8`` (ops._prec_of) and
exact fp32 under ``exact``; the rules above are fp32 FMAs.  The primal half therefore agrees with ``forward`` to the split3 tolerance, not
bit for bit (``forward`` runs the fused kernels of its launch plan).  The dual pass builds, reads and evicts no launch plan.
"""
import torch

from .. import ops
from . import image_transformer_v2 as itv2


def _layer(model, st, grids, x, xd, cond):
    """A layer step (``itv2.Step``) on the primal x and the tangent xd."""
    spec = model.level_specs[st.level].self_attn
    B, gh, gw, d = x.shape
    rps = gh * gw
    mod = st.module
    if hasattr(mod, "self_attn"):
        sa = mod.self_attn
        nh = d // spec.d_head
        h, hd = ops.rms_norm_jvp(x, xd, itv2.ada_scale(cond, sa.norm), rows_per_sample=rps)
        qkv, qkvd = ops.linear(h, sa.qkv_proj.weight), ops.linear(hd, sa.qkv_proj.weight)
        cos_t, sin_t = model._rope(st.level, grids, sa, x.device)
        ops.qk_prep_jvp_(qkv, qkvd, sa.scale.detach().contiguous(), cos_t, sin_t, nh, itv2.EPS)
        _, core, params = itv2.attn_geometry(spec, st.index)
        o, od = getattr(ops, core + "_jvp")(qkv, qkvd, nh, *params)
        x, xd = ops.linear(o, sa.out_proj.weight, residual=x), ops.linear(od, sa.out_proj.weight, residual=xd)
    ff = mod.ff
    h, hd = ops.rms_norm_jvp(x, xd, itv2.ada_scale(cond, ff.norm), rows_per_sample=rps)
    u, ud = ops.linear(h, ff.up_proj.weight), ops.linear(hd, ff.up_proj.weight)        # [value | gate] rows (linear_geglu, :89-95)
    g, gd = ops.geglu_jvp(u, ud)
    return ops.linear(g, ff.down_proj.weight, residual=x), ops.linear(gd, ff.down_proj.weight, residual=xd)


@torch.no_grad()
def forward_jvp(model, x, sigma, x_dot, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None):
    """(out, out_dot) of the inner model F (``sigma_data`` None) or of the Karras denoiser around it (``sigma_data`` given)."""
    m = model
    x, x_dot = m._check_input(x, class_cond, mapping_cond, "forward_jvp", (x_dot, m.in_channels, "tangent shape {} != input shape {}"))
    grids = m._token_grids(x)
    B = x.shape[0]
    sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    prec = ops._prec_of(x)
    pre = dict(sigma=sigma, sigma_data=float(sigma_data)) if sigma_data is not None else {}
    cond = itv2.conditioning(m, sigma, aug_cond, class_cond, mapping_cond)

    h = ops.patch_in(x, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    hd = ops.patch_in(x_dot, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    skips = []
    for st in itv2.hourglass(m):
        if st.kind == "layer":
            h, hd = _layer(m, st, grids, h, hd, cond)
        elif st.kind == "merge":
            skips.append((h, hd))
            w = m.merges[st.level].proj.weight
            h, hd = ops.token_merge(h, w), ops.token_merge(hd, w)
        else:
            sp, (s, sd) = m.splits[st.level], skips.pop()
            fac = sp.fac.detach().contiguous()
            h, hd = ops.token_split_lerp(h, sp.proj.weight, s, fac), ops.token_split_lerp(hd, sp.proj.weight, sd, fac)
    h, hd = ops.rms_norm_jvp(h, hd, m.out_norm.scale.detach().contiguous())
    w = m.patch_out.proj.weight
    skip, skip_d = (x, x_dot) if sigma_data is not None else (None, None)
    out = ops.patch_out(h, None, w, m.patch_size, m.out_channels, x_in=skip, **pre)
    out_d = ops.patch_out(hd, None, w, m.patch_size, m.out_channels, x_in=skip_d, **pre)
    return out, out_d

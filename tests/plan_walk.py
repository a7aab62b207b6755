"""A second statement of the bf16 / fp8 forward of ImageTransformerDenoiserModelV2: one public ``ops`` call per launch of the model's
launch plan, every call with a fresh output of its own.

The model's plan (models/image_transformer_v2.py: ``_Plan``) runs prebuilt descriptors over shared workspaces: in-place residual updates,
one ``qkv`` / ``att`` / ``hid`` buffer for all levels, AdaRMSNorm scales read at byte offsets of one [B, scale_width] table.  ``walk`` below
computes the same network on the same kernels with none of that: it derives its shapes from the module tree, ``hourglass(model)``,
``attn_geometry`` and ``route_layer`` (routing is mirrored, not re-decided), concatenates the AdaRMSNorm projections in an order of its own,
slices the product into contiguous [B, d] tensors and hands every op freshly allocated operands.  Same entry points, same shapes, same
operand values: the plan's output must equal the walker's bit for bit, and a wiring mistake of the plan (a wrong table offset, a wrong
workspace view, a wrong layer index, rows_per_sample or skip) changes bits.  It reads nothing of ``_Plan``.

tests/test_plan_walk_gpu.py holds the comparison; the walker itself is pinned on the CPU oracle there.
"""
import os
import sys

import torch

EPS = 1e-6


def _modules(model):
    v2 = sys.modules[type(model).__module__]
    return v2, v2.nat, v2.ops


def ada_norm_order(model):
    """(name, AdaRMSNorm module) of every norm of the network, in the walker's own order: the forward order of ``hourglass(model)``."""
    v2, _, _ = _modules(model)
    out = []
    for st in v2.hourglass(model):
        if st.kind == "layer":
            if hasattr(st.module, "self_attn"):
                out.append((st.prefix + "self_attn.norm", st.module.self_attn.norm))
            out.append((st.prefix + "ff.norm", st.module.ff.norm))
    return out


def scales(model, sigma, aug_cond=None, class_cond=None, mapping_cond=None):
    """{norm name: [B, d] fp32 scales} of every AdaRMSNorm: the conditioning chain (FourierFeatures -> mapping network -> ONE product against
    the concatenated norm projections, "+ 1" in its epilogue) on the per-row fp32 kernels the plan's chain uses."""
    _, nat, ops = _modules(model)
    m, dev, B = model, sigma.device, sigma.shape[0]
    f32 = dict(device=dev, dtype=torch.float32)

    def product(a, w, **kw):
        rows, n = a.shape[0], w.shape[0] // (2 if kw.get("epi") == nat.EPI_GEGLU else 1)
        return ops.gemm(a, w, torch.empty(rows, n, **f32), M=rows, N=n, K=w.shape[1], per_row=True, precision=nat.PREC_SPLIT3, **kw)

    temb = product(ops.fourier_sigma(sigma, m.time_emb.weight), m.time_in_proj.weight)
    if aug_cond is None:
        # aug_cond = zeros: one constant row, added to every sample
        aug_term = product(ops.fourier_features(torch.zeros(1, 9, **f32), m.aug_emb.weight), m.aug_in_proj.weight).reshape(-1)
    else:
        aug = aug_cond.to(**f32).reshape(B, 9).contiguous()
        aug_term = product(ops.fourier_features(aug, m.aug_emb.weight), m.aug_in_proj.weight)
    emb = ids = mterm = None
    if m.class_emb is not None:
        emb, ids = m.class_emb.weight, class_cond.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
    if m.mapping_cond_in_proj is not None:
        mterm = product(mapping_cond.to(**f32).reshape(B, -1).contiguous(), m.mapping_cond_in_proj.weight)
    c = ops.rms_norm(ops.cond_sum(temb, aug_term, emb=emb, ids=ids, c=mterm), m.mapping.in_norm.scale, eps=EPS)
    for blk in m.mapping.blocks:
        h = product(c, blk.up_proj.weight, epi=nat.EPI_GEGLU, norm_scale=blk.norm.scale, scale_stride=0, rows_per_sample=B)
        c = product(h, blk.down_proj.weight, epi=nat.EPI_RESIDUAL, residual=c)
    cond = ops.rms_norm(c, m.mapping.out_norm.scale, eps=EPS)
    norms = ada_norm_order(m)
    wcat = torch.cat([mod.linear.weight.detach() for _, mod in norms], dim=0).contiguous()
    table = product(cond, wcat, out_add=1.0)
    out, off = {}, 0
    for name, mod in norms:
        d = mod.linear.weight.shape[0]
        out[name] = table[:, off:off + d].contiguous()
        off += d
    assert off == table.shape[1]
    return out


def walk(model, x, sigma, *, mode, sigma_data=None, aug_cond=None, class_cond=None, mapping_cond=None, streams=None):
    """F(x, sigma) -- or, with ``sigma_data``, the Karras denoiser D(x, sigma) -- of ``model`` in arithmetic mode ``mode`` ("bf16" /
    "fp8"), one ``ops`` call per launch of the plan.  ``streams``: a dict that receives {level: the level's final residual stream}."""
    v2, nat, ops = _modules(model)
    lib = nat.lib()                                   # (also applies KDIFF_OPTIONS: route_layer reads mx8_min_rows from the library)
    prec = {"bf16": nat.PREC_BF16, "fp8": nat.PREC_FP8}[mode]
    switches = {name: os.environ.get(name, default) for name, default in v2.PLAN_SWITCHES}
    m, dev = model, x.device
    x = x.contiguous()
    B, _, H, W = x.shape
    ph, pw = m.patch_size
    levels = m.level_specs
    grids = [(H // ph, W // pw)]
    for _ in levels[1:]:
        grids.append((grids[-1][0] // 2, grids[-1][1] // 2))
    sig = sigma.to(device=dev, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    sc = scales(m, sig, aug_cond, class_cond, mapping_cond)
    pre = {} if sigma_data is None else dict(sigma=sig, sigma_data=float(sigma_data))

    cur = {0: ops.patch_in(x, m.patch_in.proj.weight, (ph, pw), precision=nat.PREC_BF16, **pre)}
    skips, seen = {}, {}
    for st in v2.hourglass(m):
        li = st.level
        if st.kind == "merge":
            skips[li] = cur[li]
            cur[li + 1] = ops.token_merge(cur[li], m.merges[li].proj.weight)
            continue
        if st.kind == "split":
            cur[li] = ops.token_split_lerp(cur[li + 1], m.splits[li].proj.weight, skips[li], m.splits[li].fac)
            continue
        lv, (gh, gw), mod, h = levels[li], grids[li], st.module, cur[li]
        d, d_ff, rps = lv.width, lv.d_ff, gh * gw
        nh = d // lv.self_attn.d_head if hasattr(mod, "self_attn") else 0
        # the layer's index is the walker's own count: an up level's layers count on from its down level's (which sets the window shift)
        index = seen.get(li, 0)
        seen[li] = index + 1
        kind, core, params = v2.attn_geometry(lv.self_attn, index) if nh else (None, None, ())
        r = v2.route_layer(lib, prec, B, B * rps, rps, d, d_ff, nh, kind, switches, grid=(gh, gw),
                           kernel_size=params[0] if kind == "neighborhood" else None)
        att = None
        if nh:
            sa, s = mod.self_attn, sc[st.prefix + "self_attn.norm"]
            qk = (sa.scale, *m._rope(li, grids, sa, dev, revs=True), nh)
            w_qkv = sa.qkv_proj.weight
            if r.qkv == "attn_block":
                att = ops.attn_block(h, s, w_qkv, rows_per_sample=rps, qk=qk, eps=EPS)
            else:
                if r.qkv == "proj_block":
                    qkv = ops.proj_block(h, s, w_qkv, rows_per_sample=rps, epi=nat.EPI_QKV, qk=qk, eps=EPS)
                elif r.qkv in ("mx8", "plain"):
                    qkv = ops.norm_linear(h, s, w_qkv, rows_per_sample=rps, epi=nat.EPI_QKV, qk=qk, eps=EPS, mx8=r.qkv == "mx8")
                else:
                    raise NotImplementedError(f"{st.prefix}: no ops form of the qkv route {r.qkv!r}")
                if r.core != f"kd_{core}_bf16":
                    raise NotImplementedError(f"{st.prefix}: no ops form of the attention core {r.core!r}")
                att = getattr(ops, core)(qkv, nh, *params)
            if not r.fuse_out:
                h = ops.linear(att, sa.out_proj.weight, residual=h)
        s, w_up, w_down = sc[st.prefix + "ff.norm"], mod.ff.up_proj.weight, mod.ff.down_proj.weight
        if r.ff == "kd_ffn_bf16":
            h = ops.ffn(h, s, w_up, w_down, rows_per_sample=rps, eps=EPS, attn=att if r.fuse_out else None,
                        w_out=mod.self_attn.out_proj.weight if r.fuse_out else None)
        elif r.ff == "pair" and not r.fuse_out and r.up in ("proj_block", "mx8", "plain"):
            if r.down_mx8:
                h8, h_scales = ops.norm_linear(h, s, w_up, rows_per_sample=rps, epi=nat.EPI_GEGLU, eps=EPS, mx8=True, c_fp8=True)
                h = ops.linear_mx8(h8, h_scales, w_down, residual=h)
            else:
                if r.up == "proj_block":
                    hid = ops.proj_block(h, s, w_up, rows_per_sample=rps, epi=nat.EPI_GEGLU, eps=EPS)
                else:
                    hid = ops.norm_linear(h, s, w_up, rows_per_sample=rps, epi=nat.EPI_GEGLU, eps=EPS, mx8=r.up == "mx8")
                h = ops.linear(hid, w_down, residual=h)
        else:
            raise NotImplementedError(f"{st.prefix}: no ops form of the FF route {r}")
        cur[li] = h
    if streams is not None:
        streams.update(cur)
    post = {} if sigma_data is None else dict(x_in=x, **pre)
    return ops.patch_out(cur[0], m.out_norm.scale, m.patch_out.proj.weight, (ph, pw), m.out_channels, eps=EPS, **post)

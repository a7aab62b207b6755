"""Backward pass (reverse-mode VJP) of the hourglass transformer w.r.t. its input: what autograd calls for ``ImageTransformerDenoiserModelV2``.

``backward(model, x, sigma, grad_out, ...)`` returns J^T grad_out for the inner model F (``sigma_data`` None) or for the Karras denoiser
D(x) = F(x c_in) c_out + x c_skip (``sigma_data`` given).  Gradient guidance (a loss on the denoised image differentiated w.r.t. x on every
solver step) and the reference's autograd form of log_likelihood (k_diffusion/sampling.py:286-294) need it.  The conditioning and the
weights are held fixed: sigma, aug_cond, class_cond, mapping_cond and the parameters get no gradient.

With ``params`` (``Denoiser.loss``: ``primal`` is its forward) the same walk also returns the gradients of those parameters.  At every
projection it holds the gradient G on the output and recomputes the operand X on the input side: dW = G^T X on ``ops.wgrad`` (csrc/wgrad_f32.hip),
the normalised operand formed in the kernel's prologue (rrms per row, the AdaRMSNorm scale per sample, GEGLU of the recomputed [value | gate]
rows).  The norms' scales, the attention scale and TokenSplit's fac reduce on ``ops.colsum``; each AdaRMSNorm's ds feeds
d cond = sum ds W_norm, which walks the mapping network back to time_in_proj, aug_in_proj, mapping_cond_in_proj and class_emb.  Parameters
not in ``params`` cost nothing; the input gradient is the same bits either way.

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
Dropout (``dropout``: the training loss's key, ``enable_dropout``): the primal masks the attention output and the FF / mapping hidden at
``itv2.dropout_sites`` in place; the reverse walk masks the gradient through each site again (dropout is its own transpose: ``ops.dropout``
on g W_out^T, the GEGLU VJP's g_h inside its kernel) and the weight gradient behind it (dW_out reads the masked o, dW_down masks its GEGLU
prologue).  No mask is stored: every kernel regenerates the bits from (key, site, element).
Arithmetic: fp32 in every KDIFF_GEMM mode, as the dual pass (split3 GEMMs under ``split3`` / ``bf16`` / ``fp8``, exact fp32 under
``exact``).  ``model.set_wgrad_arithmetic("bf16")`` moves the weight-gradient GEMMs alone (every ``ops.wgrad`` of the sink) to bf16 operands
with fp32 accumulation; the primal, the data-gradient GEMMs, the attention rules and the column sums stay as above, so the loss and the
input gradient keep their bits.  No launch plan is built, read or evicted.
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


def _attn_fwd(model, st, grids, x, cond, keep, drop=None):
    """The self-attention sublayer (:466-476) of layer step ``st`` from its input x: returns x + out_proj(attn), and with ``keep`` what
    its reverse needs (the AdaRMSNorm scale, the unprepared and the prepared qkv, the RoPE tables, the attention output as out_proj read
    it).  ``drop``: the loss call's ``itv2.dropout_table``."""
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
    dr = drop.get((st.prefix, "attn")) if drop else None
    if dr is not None:
        ops.dropout(o, *dr, out=o)
    x = ops.linear(o, sa.out_proj.weight, residual=x)
    return x, ((s, qkv, prep, cos_t, sin_t, o) if keep else None)


def _layer_fwd(model, st, grids, x, cond, drop=None):
    if hasattr(st.module, "self_attn"):
        x, _ = _attn_fwd(model, st, grids, x, cond, keep=False, drop=drop)
    ff = st.module.ff
    rps = x.shape[1] * x.shape[2]
    h = ops.norm_linear(x, itv2.ada_scale(cond, ff.norm), ff.up_proj.weight, rows_per_sample=rps, epi=ops.nat.EPI_GEGLU)
    dr = drop.get((st.prefix, "ff")) if drop else None
    if dr is not None:
        ops.dropout(h, *dr, out=h)
    return ops.linear(h, ff.down_proj.weight, residual=x)


class _Sink:
    """The parameter gradients of one reverse walk: which parameters want one (``params``), the tensors made so far (by ``id``), and the
    conditioning gradient d cond the AdaRMSNorms add up when anything behind them wants a gradient."""

    def __init__(self, model, params, cond):
        self.ids = {id(p) for p in params}
        self.grads = {}
        m = model
        behind = [m.time_in_proj.weight, m.aug_in_proj.weight, *m.mapping.parameters()]
        behind += [t.weight for t in (m.class_emb, m.mapping_cond_in_proj) if t is not None]
        self.chain = self.wants(*behind)
        self.cond = cond
        self.dcond = None
        self.bf16 = model.wgrad_arithmetic == "bf16"

    def wgrad(self, G, A, **kw):
        """``ops.wgrad`` in the model's weight-gradient arithmetic (``set_wgrad_arithmetic``)."""
        return ops.wgrad(G, A, bf16=self.bf16, **kw)

    def wants(self, *ps):
        return any(id(p) in self.ids for p in ps)

    def put(self, p, make):
        if id(p) in self.ids:
            self.grads[id(p)] = make()

    def ada(self, model, norm, gy, x, rrms, rps):
        """AdaRMSNorm y = x rrms (cond W^T + 1) with gradient gy on y: dW = ds^T cond and d cond += ds W, ds[b, j] = sum over sample b's
        rows of gy x rrms."""
        if not (self.chain or self.wants(norm.linear.weight)):
            return
        ds = ops.colsum(gy, x, row_scale=rrms, rows_per_seg=rps)
        self.put(norm.linear.weight, lambda: self.wgrad(ds, self.cond))
        if self.chain:
            self.dcond = ops.linear(ds, _wt(model, norm.linear.weight), residual=self.dcond)


def _layer_vjp(model, st, grids, x, g, cond, sink=None, drop=None):
    """Gradient w.r.t. the input x of layer step ``st`` from the gradient g on its output; the layer's insides are recomputed from x.  With
    ``sink`` the layer's parameter gradients go there too.  ``drop``: the loss call's ``itv2.dropout_table`` -- each mask applies again to
    the gradient through its site (dropout is its own transpose) and to the operand of the weight gradient behind it."""
    B, gh, gw, d = x.shape
    rps = gh * gw
    has_attn = hasattr(st.module, "self_attn")
    if has_attn:
        xf, (s_a, qkv, prep, cos_t, sin_t, o) = _attn_fwd(model, st, grids, x, cond, keep=True, drop=drop)
    else:
        xf = x
    ff = st.module.ff
    d_ff = drop.get((st.prefix, "ff")) if drop else None
    s_f = itv2.ada_scale(cond, ff.norm)
    u = ops.norm_linear(xf, s_f, ff.up_proj.weight, rows_per_sample=rps)           # [value | gate] rows (linear_geglu, :89-95)
    gu = ops.geglu_vjp(u, ops.linear(g, _wt(model, ff.down_proj.weight)), dropout=d_ff)      # g_h = mask (g W_down^T) into the GEGLU VJP
    gy = ops.linear(gu, _wt(model, ff.up_proj.weight))
    if sink is not None:
        sink.put(ff.down_proj.weight, lambda: sink.wgrad(g, u, geglu=True, dropout=d_ff))      # g^T (mask geglu(u))
        r = ops.row_rrms(xf, itv2.EPS) if sink.wants(ff.up_proj.weight, ff.norm.linear.weight) or sink.chain else None
        sink.put(ff.up_proj.weight, lambda: sink.wgrad(gu, xf, row_scale=r, col_scale=s_f, rows_per_sample=rps))
        sink.ada(model, ff.norm, gy, xf, r, rps)
    g = ops.rms_norm_vjp(xf, gy, s_f, rows_per_sample=rps, add=g)
    if not has_attn:
        return g
    sa = st.module.self_attn
    spec = model.level_specs[st.level].self_attn
    nh = d // spec.d_head
    go = ops.linear(g, _wt(model, sa.out_proj.weight))
    d_attn = drop.get((st.prefix, "attn")) if drop else None
    if d_attn is not None:
        ops.dropout(go, *d_attn, out=go)
    if sink is not None:
        sink.put(sa.out_proj.weight, lambda: sink.wgrad(g, o))                           # o: already masked by the recomputation
    _, core, params = itv2.attn_geometry(spec, st.index)
    gq = getattr(ops, core + "_vjp")(prep, go, nh, *params)
    scale = sa.scale.detach().contiguous()
    if sink is not None:
        sink.put(sa.scale, lambda: ops.attn_scale_grad(ops.colsum(gq, prep), scale, nh))
    ops.qk_prep_vjp_(qkv, gq, scale, cos_t, sin_t, nh, itv2.EPS)
    gy = ops.linear(gq, _wt(model, sa.qkv_proj.weight))
    if sink is not None:
        r = ops.row_rrms(x, itv2.EPS) if sink.wants(sa.qkv_proj.weight, sa.norm.linear.weight) or sink.chain else None
        sink.put(sa.qkv_proj.weight, lambda: sink.wgrad(gq, x, row_scale=r, col_scale=s_a, rows_per_sample=rps))
        sink.ada(model, sa.norm, gy, x, r, rps)
    return ops.rms_norm_vjp(x, gy, s_a, rows_per_sample=rps, add=g)


def _mapping_vjp(m, keep, sink, drop=None):
    """The conditioning chain in reverse (image_transformer_v2.py:729-740, :552-581) from d cond on its output: the mapping network's
    norms and blocks (their GEGLU outputs under ``drop``'s mapping sites), then the projections of the Fourier features and mapping_cond,
    and the class embedding."""
    mp = m.mapping
    dc = sink.dcond
    B = dc.shape[0]
    c = keep["c_last"]
    if sink.wants(mp.out_norm.scale):
        sink.put(mp.out_norm.scale, lambda: ops.colsum(dc, c, row_scale=ops.row_rrms(c, itv2.EPS)).reshape(-1))
    dc = ops.rms_norm_vjp(c, dc, mp.out_norm.scale.detach().contiguous())
    for k, blk, c in reversed(list(zip(range(len(mp.blocks)), mp.blocks, keep["blocks"]))):
        dk = drop.get(("mapping", k)) if drop else None
        nscale = blk.norm.scale.detach().contiguous()
        u = ops.norm_linear(c, blk.norm.scale, blk.up_proj.weight, rows_per_sample=B)
        gu = ops.geglu_vjp(u, ops.linear(dc, _wt(m, blk.down_proj.weight)), dropout=dk)
        gy = ops.linear(gu, _wt(m, blk.up_proj.weight))
        r = ops.row_rrms(c, itv2.EPS)
        sink.put(blk.down_proj.weight, lambda: sink.wgrad(dc, u, geglu=True, dropout=dk))
        sink.put(blk.up_proj.weight, lambda: sink.wgrad(gu, c, row_scale=r, col_scale=nscale))
        sink.put(blk.norm.scale, lambda: ops.colsum(gy, c, row_scale=r).reshape(-1))
        dc = ops.rms_norm_vjp(c, gy, nscale, add=dc)
    c0 = keep["c_sum"]
    sink.put(mp.in_norm.scale, lambda: ops.colsum(dc, c0, row_scale=ops.row_rrms(c0, itv2.EPS)).reshape(-1))
    dc = ops.rms_norm_vjp(c0, dc, mp.in_norm.scale.detach().contiguous())
    sink.put(m.time_in_proj.weight, lambda: sink.wgrad(dc, keep["time_ff"]))
    sink.put(m.aug_in_proj.weight, lambda: sink.wgrad(dc, keep["aug_ff"]))
    if m.mapping_cond_in_proj is not None:
        sink.put(m.mapping_cond_in_proj.weight, lambda: sink.wgrad(dc, keep["mapping_rows"]))
    if m.class_emb is not None:
        sink.put(m.class_emb.weight, lambda: ops.class_emb_grad(dc, keep["ids"], m.class_emb.weight.shape[0]))


def _primal(m, x, grids, cond, pre, prec, drop=None):
    """The fp32 ``ops``-path primal up to the output norm (image_transformer_v2.py:721-758): (h, every layer's input, every merge's input,
    every split's input)."""
    acts, skips, merge_in, split_in = [], [], [], []
    h = ops.patch_in(x, m.patch_in.proj.weight, m.patch_size, precision=prec, **pre)
    for st in itv2.hourglass(m):
        if st.kind == "layer":
            acts.append(h)
            h = _layer_fwd(m, st, grids, h, cond, drop)
        elif st.kind == "merge":
            skips.append(h)
            merge_in.append(h)
            h = ops.token_merge(h, m.merges[st.level].proj.weight)
        else:
            sp = m.splits[st.level]
            split_in.append(h)
            h = ops.token_split_lerp(h, sp.proj.weight, skips.pop(), sp.fac.detach().contiguous())
    return h, acts, merge_in, split_in


@torch.no_grad()
def primal(model, x, sigma, aug_cond=None, class_cond=None, mapping_cond=None, dropout=None):
    """F(x, sigma) of the inner model on the fp32 ``ops`` path (what ``backward`` recomputes; no launch plan is built, read or evicted).
    ``dropout``: the loss call's key (a one-element int64 device tensor) -- the model's dropout sites (``itv2.dropout_sites``) mask their
    tensors; None: no dropout."""
    m = model
    x, _ = m._check_input(x, class_cond, mapping_cond, "the training loss")
    grids = m._token_grids(x)
    B = x.shape[0]
    sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    drop = itv2.dropout_table(m, dropout)
    cond = itv2.conditioning(m, sigma, aug_cond, class_cond, mapping_cond, drop=drop)
    h, *_ = _primal(m, x, grids, cond, {}, ops._prec_of(x), drop)
    return ops.patch_out(h, m.out_norm.scale.detach().contiguous(), m.patch_out.proj.weight, m.patch_size, m.out_channels)


@torch.no_grad()
def backward(model, x, sigma, grad_out, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None, params=None, dropout=None):
    """J^T grad_out w.r.t. x of the inner model F (``sigma_data`` None) or of the Karras denoiser around it (``sigma_data`` given).  With
    ``params`` (a list of the model's parameters; inner model only): (J^T grad_out, {id(p): gradient of p}) -- the input gradient is the
    same bits as without.  ``dropout``: the key ``primal`` ran with (the same masks are regenerated), or None."""
    m = model
    x, grad_out = m._check_input(x, class_cond, mapping_cond, "the backward pass",
                                 (grad_out, m.out_channels, "gradient shape {} != output shape {}"))
    if params is not None and sigma_data is not None:
        raise ValueError("backward: parameter gradients are taken through the inner model only (sigma_data None)")
    grids = m._token_grids(x)
    B = x.shape[0]
    sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
    prec = ops._prec_of(x)
    pre = dict(sigma=sigma, sigma_data=float(sigma_data)) if sigma_data is not None else {}
    keep = {} if params is not None else None
    drop = itv2.dropout_table(m, dropout)
    cond = itv2.conditioning(m, sigma, aug_cond, class_cond, mapping_cond, keep=keep, drop=drop)
    sink = _Sink(m, params, cond) if params is not None else None
    steps = itv2.hourglass(m)

    # primal, keeping every layer's input (image_transformer_v2.py:721-762)
    h, acts, merge_in, split_in = _primal(m, x, grids, cond, pre, prec, drop)

    # reverse walk
    g_img = ops.precond_vjp(grad_out, ops.nat.PC_OUT, sigma, sigma_data) if sigma_data is not None else grad_out
    g = ops.patch_in(g_img, _wt(m, m.patch_out.proj.weight), m.patch_size, precision=prec)     # patch-out^T: the patch gather
    out_scale = m.out_norm.scale.detach().contiguous()
    if sink is not None and sink.wants(m.patch_out.proj.weight, m.out_norm.scale):
        gh, gw = grids[0]
        ph, pw = m.patch_size
        r = ops.row_rrms(h, itv2.EPS)
        sink.put(m.patch_out.proj.weight, lambda: sink.wgrad(g_img, h, gather=("g", ops.nat.WG_PATCH_NCHW), gather_geom=(gh, gw, ph, pw, m.out_channels),
                                                            row_scale=r, col_scale=out_scale))
        sink.put(m.out_norm.scale, lambda: ops.colsum(g, h, row_scale=r).reshape(-1))
    g = ops.rms_norm_vjp(h, g, out_scale)
    del h
    g_skips = []
    for st in reversed(steps):
        if st.kind == "layer":
            g = _layer_vjp(m, st, grids, acts.pop(), g, cond, sink, drop)
        elif st.kind == "split":
            sp = m.splits[st.level]
            xs = split_in.pop()
            if sink is not None:
                skip = merge_in[st.level]
                _, _, one = _split_consts(m, sp, B, x.device)
                gh, gw = xs.shape[1:3]
                sink.put(sp.proj.weight, lambda: sink.wgrad(g, xs, gather=("g", ops.nat.WG_MERGE2x2), gather_geom=(gh, gw, 2, 2, skip.shape[-1]),
                                                           alpha=sp.fac.detach().contiguous()))
                if sink.wants(sp.fac):                                                 # d fac = sum g (split(x) - skip)
                    y = ops.token_split_lerp(xs, sp.proj.weight, skip, one)
                    sink.put(sp.fac, lambda: ops.colsum(ops.colsum(g, y, b2=skip).reshape(-1, 1)).reshape(1))
            g_skips.append(g)                                                          # the skip's share: (1 - fac) g, taken at the merge
            g = ops.token_merge(g, _wt(m, sp.proj.weight, fac=sp.fac))
        else:
            omf, ones, one = _split_consts(m, m.splits[st.level], B, x.device)
            gs = g_skips.pop()
            xm = merge_in.pop()
            if sink is not None:
                gh, gw = g.shape[1:3]
                sink.put(m.merges[st.level].proj.weight, lambda: sink.wgrad(g, xm, gather=("a", ops.nat.WG_MERGE2x2),
                                                                          gather_geom=(gh, gw, 2, 2, xm.shape[-1])))
            g = ops.token_split_lerp(g, _wt(m, m.merges[st.level].proj.weight), gs, one)     # TokenMerge^T: depth-to-space (lerp weight 1)
            g = ops.rows_affine(gs, omf, g, ones)
    if sink is not None:
        gh, gw = grids[0]
        ph, pw = m.patch_size
        sink.put(m.patch_in.proj.weight, lambda: sink.wgrad(g, x, gather=("a", ops.nat.WG_PATCH_NCHW), gather_geom=(gh, gw, ph, pw, m.in_channels)))
        if sink.chain:
            _mapping_vjp(m, keep, sink, drop)
    g = ops.patch_out(g, None, _wt(m, m.patch_in.proj.weight), m.patch_size, m.in_channels)   # patch-in^T: the un-patch
    if sigma_data is not None:
        g = ops.precond_vjp(g, ops.nat.PC_IN, sigma, sigma_data, h=grad_out, h_coef=ops.nat.PC_SKIP)
    return g if sink is None else (g, sink.grads)

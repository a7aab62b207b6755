"""Reverse pass (VJP) of the image_v1 U-Net w.r.t. its input: ``ImageDenoiserModelV1.forward_vjp`` in the shape of ``torch.func.vjp``.

``forward_vjp(model, x, sigma, ...)`` returns ``(out, pullback)``: out = F(x, sigma) -- or the Karras denoiser D(x, sigma) with ``sigma_data``, the
scalings folded into ``proj_in`` / ``proj_out`` as in ``forward_preconditioned`` -- with the forward's bits, and ``pullback(grad_out)`` =
J^T grad_out.  Gradient guidance (a loss on the denoised image differentiated w.r.t. x on every solver step) needs it.  sigma, the
conditioning and the weights are held fixed and get no gradient: the contract of ``models/vjp.py``.

Recompute, do not save.  The primal issues the forward plan's kernels with the same operands in the same order, but on tensors of its own (a
pullback may be called long after, and more than once), keeping one tensor per layer input -- the skips are the right halves of the concat
buffers -- and the AdaGN table.  The pullback walks the tape in reverse and recomputes inside a layer what its reverse needs when it gets there:
the pre-norm t2 of a residual block, the qkv of an attention layer, the group statistics.
  - a convolution's data gradient is the same kernel on the transposed, flipped weight (``unet_ops.conv2d_dgrad``), the q rows of the qkv
    weight with their folded 1 / 8; the bias gets none; the kernel's residual epilogue is not needed: every sum of two gradients falls into
    AdaGN's ``g_add`` (a block's input feeds its first AdaGN and its skip) or the resamplers' accumulate flag;
  - AdaGN (+ GELU) and the two resamplers have HIP rules of their own (csrc/unet_vjp_f32.hip), attention is ``ops.attn_global_vjp``;
  - ``torch.cat([x, skip])`` in reverse is two column ranges of the gradient of the block that read it: the left goes through up2's transpose,
    the right takes the sum with down2's transpose and is the gradient of the down path's output at that level;
  - the ends are each other's transposes: proj_out^T is ``unet_in`` with the transposed weight, proj_in^T is ``unet_out``, and the
    preconditioning's per-sample scalings go through ``ops.precond_vjp``.
fp32-grade arithmetic whatever ``KDIFF_GEMM`` says, like the forward.  No launch plan of the forward or the dual pass is built, read or evicted:
the few weight-derived tensors of this pass (the mappers' concatenated weight, the folded qkv weights, the transposed projections) live in a
cache of their own, dropped when the weights fingerprint moves.

``drop`` (the training loss in training mode after ``enable_dropout()``, models/unet_train.py: ``make_drop``; ``forward_vjp`` never passes
one): the key of the loss call, the table of channel factors and every layer's site.  The channel masks ride in the epilogues of the two
convolutions of a residual block (``kd_conv2d_x3_drop``), in the primal and in the recomputation alike; in reverse the gradient takes the
mask's transpose (``unet_ops.chan_scale``) in front of each convolution's three consumers, and attention runs its dropout kernels.  None: the
launches are the ones they were.
"""
from types import SimpleNamespace

import torch
from torch import nn

from .. import ops
from .. import unet_ops as uo
from . import image_v1 as v1

MAX_CONSTS = 2      # devices whose weight-derived tensors are kept per model


class _Consts:
    """What this pass derives from the weights alone, on one device."""

    def __init__(self, model):
        norms = [m for m in model.u_net.modules() if isinstance(m, v1._AdaGN)]
        self.map_w = torch.cat([m.mapper.weight.detach() for m in norms]).contiguous()
        self.map_b = torch.cat([m.mapper.bias.detach() for m in norms]).contiguous()
        self.offsets, off = {}, 0
        for m in norms:
            self.offsets[m] = off
            off += 2 * m.c_out
        self.qkv = {}
        for layer in model.u_net.modules():
            if isinstance(layer, v1._SelfAttention2d):              # the forward's folding: 1 / 8 into the q rows, exactly
                wq, bq = layer.qkv_proj.weight.detach().clone(), layer.qkv_proj.bias.detach().clone()
                wq[:layer.c_in] *= 0.125
                bq[:layer.c_in] *= 0.125
                self.qkv[layer] = (wq, bq, uo.pack_conv(wq, cache=False))
        c_img, ch = model.c_in, model.channels[0]
        self.out_t = model.proj_out.weight.detach().reshape(c_img, ch).t().contiguous()      # [C, c_img]: proj_out^T on unet_in
        self.in_t = model.proj_in.weight.detach().reshape(ch, c_img).t().contiguous()        # [c_img, C]: proj_in^T on unet_out


def _consts(model, fingerprint, device):
    if fingerprint != model._vjp_fingerprint:
        model._vjp_cache.drop_all()
        model._vjp_fingerprint = fingerprint
    key = str(device)
    return model._vjp_cache.get(key) or model._vjp_cache.put(key, lambda: _Consts(model), MAX_CONSTS)


def _empty(like, rows, cols):
    return torch.empty(rows, cols, device=like.device, dtype=torch.float32)


def _wb(c, norm):
    off = c.consts.offsets[norm]
    return c.table[:, off:off + 2 * norm.c_out]


def _res_front(c, layer, x, hw, drop=None):
    """A residual block up to its second norm: (statistics of x, the first convolution's input t1, the pre-norm t2 -- behind the first
    Dropout2d with ``drop``: the second norm's statistics see the mask)."""
    norm = layer.main[0]
    stats = uo.groupnorm_stats(x, c.B, norm.num_groups, norm.eps)
    t1 = uo.adagn_apply(x, stats, _wb(c, norm), gelu=True)
    t2 = uo.conv2d(t1, layer.main[2].weight, c.B, *hw, bias=layer.main[2].bias, chan_scale=None if drop is None else drop.chan[layer][0])
    return stats, t1, t2


def _res_fwd(c, layer, x, y, hw, drop=None):
    _, _, t2 = _res_front(c, layer, x, hw, drop)
    norm = layer.main[4]
    uo.adagn_apply(t2, uo.groupnorm_stats(t2, c.B, norm.num_groups, norm.eps), _wb(c, norm), gelu=True, out=t2)
    res = uo.conv2d(x, layer.skip.weight, c.B, *hw) if isinstance(layer.skip, nn.Conv2d) else x
    uo.conv2d(t2, layer.main[6].weight, c.B, *hw, bias=layer.main[6].bias, residual=res, out=y,
              chan_scale=None if drop is None else drop.chan[layer][1])


def _res_vjp(c, layer, x, g, hw, sink=None, drop=None):
    """The gradient of a residual block's input from the gradient g of its output.  ``sink`` (the training backward, models/unet_train.py) is
    shown every gradient a parameter of the block hangs on, beside the activation that met it in the forward; without one the launches are
    ``forward_vjp``'s.  With ``drop`` the second convolution's three consumers read m2 g from a buffer of its own (the skip path keeps g), and
    the gradient that leaves the second norm is masked in place with m1 in front of the first convolution's."""
    stats0, t1, t2 = _res_front(c, layer, x, hw, drop)
    n0, n4 = layer.main[0], layer.main[4]
    stats4 = uo.groupnorm_stats(t2, c.B, n4.num_groups, n4.eps)
    g_m = g if drop is None else uo.chan_scale(g, drop.chan[layer][1], c.B)      # the gradient behind the second Dropout2d: a new buffer
    if sink is not None:
        sink.conv(layer.main[6], g_m, lambda: uo.adagn_apply(t2, stats4, _wb(c, n4), gelu=True), hw)
        if isinstance(layer.skip, nn.Conv2d):
            sink.conv(layer.skip, g, lambda: x, hw)
    g2 = uo.conv2d_dgrad(g_m, layer.main[6].weight, c.B, *hw)
    if sink is not None:
        sink.norm(n4, t2, stats4, g2, gelu=True)
    uo.adagn_vjp_apply(t2, stats4, uo.adagn_vjp_stats(t2, stats4, _wb(c, n4), g2, gelu=True), _wb(c, n4), g2, gelu=True, out=g2)
    if drop is not None:
        uo.chan_scale(g2, drop.chan[layer][0], c.B, out=g2)
    if sink is not None:
        sink.conv(layer.main[2], g2, lambda: t1, hw)
    g1 = uo.conv2d_dgrad(g2, layer.main[2].weight, c.B, *hw)
    if sink is not None:
        sink.norm(n0, x, stats0, g1, gelu=True)
    g_skip = uo.conv2d_dgrad(g, layer.skip.weight, c.B, *hw) if isinstance(layer.skip, nn.Conv2d) else g
    return uo.adagn_vjp_apply(x, stats0, uo.adagn_vjp_stats(x, stats0, _wb(c, n0), g1, gelu=True), _wb(c, n0), g1, g_add=g_skip, gelu=True, out=g1)


def _attn_front(c, layer, x, hw):
    """An attention layer up to its qkv: (statistics of x, the projection's input t1, qkv [B, H W, 3 C] with the folded q)."""
    norm = layer.norm_in
    stats = uo.groupnorm_stats(x, c.B, norm.num_groups, norm.eps)
    t1 = uo.adagn_apply(x, stats, _wb(c, norm), gelu=False)
    wq, bq, packed = c.consts.qkv[layer]
    qkv = uo.conv2d(t1, wq, c.B, *hw, bias=bq, packed=packed)
    return stats, t1, qkv.view(c.B, hw[0] * hw[1], 3 * layer.c_in)


def _attn_core(layer, q3, drop):
    """softmax(q k^T) v on the folded qkv; with ``drop`` the dropout on the probabilities at the layer's site."""
    if drop is None:
        return ops.attn_global(q3, layer.n_head)
    return uo.attn_global_drop(q3, layer.n_head, drop.key, drop.attn[layer], drop.p)


def _attn_fwd(c, layer, x, y, hw, drop=None):
    _, _, q3 = _attn_front(c, layer, x, hw)
    a = _attn_core(layer, q3, drop)
    uo.conv2d(a.view(-1, layer.c_in), layer.out_proj.weight, c.B, *hw, bias=layer.out_proj.bias, residual=x, out=y)


def _attn_vjp(c, layer, x, g, hw, sink=None, drop=None):
    """The gradient of an attention layer's input from the gradient g of its output; ``sink`` as in ``_res_vjp``.  With ``drop`` the recomputed
    attention output (out_proj's activation) and the reverse rule carry the probabilities' mask."""
    stats, t1, q3 = _attn_front(c, layer, x, hw)
    norm, C = layer.norm_in, layer.c_in
    if sink is not None:
        sink.conv(layer.out_proj, g, lambda: _attn_core(layer, q3, drop).view(-1, C), hw)
    ga = uo.conv2d_dgrad(g, layer.out_proj.weight, c.B, *hw)
    if drop is None:
        gq = ops.attn_global_vjp(q3, ga.view(c.B, hw[0] * hw[1], C), layer.n_head)
    else:
        gq = uo.attn_global_drop_vjp(q3, ga.view(c.B, hw[0] * hw[1], C), layer.n_head, drop.key, drop.attn[layer], drop.p)
    if sink is not None:                                                # gq is the gradient of the FOLDED projection's output: q rows / 8
        sink.conv(layer.qkv_proj, gq.view(-1, 3 * C), lambda: t1, hw, q_rows=C)
    g1 = uo.conv2d_dgrad(gq.view(-1, 3 * C), layer.qkv_proj.weight, c.B, *hw, q_rows=C)
    if sink is not None:
        sink.norm(norm, x, stats, g1, gelu=False)
    return uo.adagn_vjp_apply(x, stats, uo.adagn_vjp_stats(x, stats, _wb(c, norm), g1), _wb(c, norm), g1, g_add=g, out=g1)


def _primal(model, c, t0, sizes, drop=None):
    """The forward plan's walk (``image_v1._Plan``) on tensors of this call: (the last activation, the tape of steps with every layer's input)."""
    n, ch, B = len(model.depths), model.channels, c.B
    tape, cur, cats = [], t0, [None] * n

    def run(layer, x, y, hw):
        (_res_fwd if isinstance(layer, v1._ResConvBlock) else _attn_fwd)(c, layer, x, y, hw, drop)
        tape.append(("layer", layer, x, hw))
        return y
    for i, block in enumerate(model.u_net.d_blocks):
        hw = sizes[i]
        rows = B * hw[0] * hw[1]
        if i > 0:
            cur = uo.down2(cur, B, *sizes[i - 1])
            tape.append(("down", i))
        layers = list(block)[1:]
        for j, layer in enumerate(layers):
            if j == len(layers) - 1 and i < n - 1:                      # the level's skip: the right half of the up path's concat buffer
                cats[i] = _empty(t0, rows, 2 * ch[i])
                dst = cats[i][:, ch[i]:]
            else:
                dst = _empty(t0, rows, layer.c_out)
            cur = run(layer, cur, dst, hw)
    for k, block in enumerate(model.u_net.u_blocks):
        i = n - 1 - k
        hw = sizes[i]
        if i < n - 1:
            cur = cats[i]                                               # [upsampled | skip]
        for layer in list(block)[:-1]:
            cur = run(layer, cur, _empty(t0, B * hw[0] * hw[1], layer.c_out), hw)
        if i > 0:
            uo.up2(cur, B, *hw, out=cats[i - 1][:, :ch[i - 1]])
            tape.append(("up", i))
    return cur, tape


def _reverse(model, c, tape, g, sizes, sink=None, drop=None):
    """The gradient of the first activation from the gradient g of the last, along the tape in reverse; ``sink`` as in ``_res_vjp``, ``drop``
    the primal's."""
    ch, B = model.channels, c.B
    g_cat = {}                                                          # level -> gradient of its concat buffer [rows, 2 C]
    for step in reversed(tape):
        if step[0] == "layer":
            _, layer, x, hw = step
            g = (_res_vjp if isinstance(layer, v1._ResConvBlock) else _attn_vjp)(c, layer, x, g, hw, sink, drop)
        elif step[0] == "up":                                           # g: the concat buffer's; its left half came from up2
            i = step[1]
            g_cat[i - 1] = g
            g = uo.up2_vjp(g[:, :ch[i - 1]], B, *sizes[i])
        else:                                                           # down2 read the skip: its transpose adds to the right half
            i = step[1]
            right = g_cat.pop(i - 1)[:, ch[i - 1]:]
            g = uo.down2_vjp(g, B, *sizes[i - 1], out=right, accumulate=True)
    return g


def forward_vjp(model, input, sigma, mapping_cond=None, sigma_data=None, **kwargs):
    """(out, pullback) of ``model`` (an ``ImageDenoiserModelV1``): see the module docstring."""
    model._refuse(input, sigma, mapping_cond, **kwargs)
    with torch.no_grad():
        x = input.contiguous()
        B, _, H, W = x.shape
        sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        sizes = v1.level_sizes(model, H, W)
        fingerprint = model._weights_fingerprint()
        consts = _consts(model, fingerprint, x.device)
        feats = model.feats_in
        ws = SimpleNamespace(map_w=consts.map_w, map_b=consts.map_b, table=_empty(x, B, consts.map_w.shape[0]),
                             **{name: _empty(x, B, feats) for name in ("ff", "e", "h1", "h2")})
        c = SimpleNamespace(B=B, consts=consts, table=model._cond_table(sigma, mapping_cond, B, x.device, ws))
        pre = sigma_data is not None
        sigma_data = float(sigma_data) if pre else 1.0
        scale = dict(sigma=sigma if pre else None, sigma_data=sigma_data)
        t0 = uo.unet_in(x, model.proj_in.weight, model.proj_in.bias, **scale)
        last, tape = _primal(model, c, t0, sizes)
        out = uo.unet_out(last, model.proj_out.weight, model.proj_out.bias, tuple(x.shape), image=x if pre else None, **scale)

    def pullback(grad_out):
        """J^T grad_out w.r.t. the input of the primal above; grad_out has the output's shape."""
        if not isinstance(grad_out, torch.Tensor) or grad_out.shape != out.shape:
            raise ValueError(f"image_v1: grad_out has the output's shape {tuple(out.shape)} (got {tuple(getattr(grad_out, 'shape', ()))})")
        if grad_out.device != out.device:
            raise RuntimeError(f"image_v1: grad_out is on {grad_out.device}, the output on {out.device}")
        if grad_out.dtype != torch.float32:
            raise TypeError(f"image_v1: grad_out is fp32 like the output (got {grad_out.dtype})")
        if model._weights_fingerprint() != fingerprint:
            raise RuntimeError("image_v1: the model's weights changed since the forward_vjp call this pullback belongs to (its weights "
                               "fingerprint moved), and the pullback recomputes from them; call forward_vjp again")
        with torch.no_grad():
            go = grad_out.detach().contiguous()
            g_img = ops.precond_vjp(go, ops.nat.PC_OUT, sigma, sigma_data) if pre else go
            g = uo.unet_in(g_img, consts.out_t)                          # proj_out^T: NCHW -> tokens
            g = _reverse(model, c, tape, g, sizes)
            g = uo.unet_out(g, consts.in_t, None, tuple(x.shape))        # proj_in^T: tokens -> NCHW
            if pre:
                g = ops.precond_vjp(g, ops.nat.PC_IN, sigma, sigma_data, h=go, h_coef=ops.nat.PC_SKIP)
        return g
    return out, pullback

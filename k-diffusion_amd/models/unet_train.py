"""Training pass of the image_v1 U-Net: ``ImageDenoiserModelV1.loss_forward`` -- what ``Denoiser.loss`` calls -- as an autograd node whose
differentiable inputs are the model's parameters, and the parameter gradients behind it.

The node's forward is the primal of ``models/unet_vjp.py`` (the forward plan's kernels on tensors of the call's own) and keeps its tape: one
tensor per layer input and the conditioning chain's few rows.  Its backward walks that tape with ``unet_vjp._reverse`` and a *sink*: at every
layer the walk shows the sink the gradient a parameter hangs on beside the activation that met it in the forward, and the sink launches the
gradient kernel if autograd asked for that parameter (``needs_input_grad``) -- a frozen parameter costs no launch.  The tape is freed after
the backward; a second backward through a retained graph recomputes it.

  - a convolution's weight gradient is ``kd_conv2d_wgrad_x3`` (csrc/conv_wgrad_x3.hip) for ks = 3 AND for ks = 1: the 1 x 1 convolutions (skip,
    qkv_proj, out_proj) read column ranges of concat buffers, which the kernel takes through its row strides and ``ops.wgrad`` does not; its
    bias gradient is ``kd_bias_grad_f32``.  The qkv projection runs with 1 / 8 folded into its q rows, so the gradient of the STORED q weight and
    bias is 1 / 8 of the folded one (``q_rows`` / ``q_cols``);
  - AdaGN hands the gradient of its per-sample (weight, bias) pair to its column range of one table [B, sum of 2 C] (``kd_adagn_wb_grad_f32``);
    the conditioning chain behind the table has B rows: every mapper's weight gradient is a row range of ONE ``ops.wgrad`` of the table against
    the mapping network's output, the biases are ``ops.colsum``; the way back through the mappers is one more ``ops.wgrad`` (the sum over all
    mappers' columns is long), through ``mapping`` it is ``unet_ops.cond_mlp`` on the transposed weights and ``kd_gelu_vjp_f32`` at the
    recomputed pre-activations.  ``timestep_embed.weight`` is a buffer and gets none;
  - ``proj_out`` / ``proj_in`` have 1 .. 4 image channels on one side: ``ops.wgrad`` with the NCHW gather (a 1 x 1 patch) on the image operand.
    ``loss_forward`` receives the input already scaled by c_in, so no preconditioning is folded in.

Arithmetic is fp32-grade (split-bf16 x 3 on the matrix cores, fp64 sums in the small rules) whatever ``KDIFF_GEMM`` says.  x, sigma and the
conditioning get no gradient.

``model.set_wgrad_arithmetic("bf16")`` moves every weight-gradient PRODUCT, and nothing else, to bf16 operands with fp32 accumulation: the
convolutions' go to ``kd_conv2d_wgrad_bf16`` (csrc/conv_wgrad_bf16.hip; ks = 3 and ks = 1), the GEMMs of the mappers, ``mapping``,
``mapping_cond``, ``proj_in`` and ``proj_out`` to ``ops.wgrad(bf16=True)``.  The primal (so the loss bits), the data-gradient convolutions,
AdaGN and its (w, b) sums, the bias gradients, the attention rules, ``g_table map_w`` (the way back through the mappers: a data gradient that
uses ``ops.wgrad``) and the dropout masks stay as they are.

Dropout (training mode, ``dropout_rate > 0``, after ``model.enable_dropout()``; refused without it): ``loss_forward`` draws one int64 key on
the device per call -- no host sync -- and hands it to the node as a saved input, so a second backward through a retained graph recomputes
with the same masks.  ``make_drop`` fills the factors of ALL channel sites (two Dropout2d per residual block) in one ``kd_chan_mask_f32`` launch
into a table [B, sum of C]; the convolutions of the primal and of the backward's recomputation apply them in their epilogues
(``kd_conv2d_x3_drop``), the reverse walk applies the transpose with ``kd_chan_scale_f32`` (the weight-, bias- and AdaGN-gradient kernels
take no mask), and the attention layers drop probabilities in ``kd_attn_global_drop_f32`` / ``kd_attn_global_drop_vjp_f32``.  No mask is
stored: every consumer regenerates it from (key, site).  Contract: include/kdiff_unet_drop.h; sites: ``image_v1.dropout_sites``.
``model.eval()`` and a rate of 0 take no key and no table and launch what they launched before.
"""
from types import SimpleNamespace

import torch
from torch import nn

from .. import ops
from .. import unet_ops as uo
from . import image_v1 as v1
from . import unet_vjp as uv

_X3 = ops.nat.PREC_SPLIT3


def _wgrad(G, A, bf16=False, **kw):
    """A weight-gradient GEMM dW = G^T A: split3, or (``set_wgrad_arithmetic("bf16")``) both operands rounded once to bf16."""
    return ops.wgrad(G, A, precision=_X3, bf16=bf16, **kw)


class _TrainConsts:
    """The transposed weights of the conditioning chain's way back, on one device (derived once per weights fingerprint)."""

    def __init__(self, model, consts):
        self.m2_t = model.mapping[2].weight.detach().t().contiguous()
        self.m0_t = model.mapping[0].weight.detach().t().contiguous()


def _train_consts(model, consts):
    if getattr(consts, "train", None) is None:
        consts.train = _TrainConsts(model, consts)
    return consts.train


class _Sink:
    """Receives, along the reverse walk, (gradient, activation) of every parameter site and launches what ``want`` asks for."""

    def __init__(self, model, c, want):
        self.c, self.want, self.grads = c, {id(p) for p in want}, {}
        self.bf16 = model.wgrad_arithmetic == "bf16"                   # the weight-gradient products alone; every other rule stays fp32-grade
        norms = list(c.consts.offsets)
        chain = [model.mapping[0].weight, model.mapping[0].bias, model.mapping[2].weight, model.mapping[2].bias]
        if hasattr(model, "mapping_cond"):
            chain.append(model.mapping_cond.weight)
        self.chain = any(id(p) in self.want for p in chain)           # something behind the table: every norm's (w, b) gradient is needed
        self.mappers = any(id(m.mapper.weight) in self.want or id(m.mapper.bias) in self.want for m in norms)
        self.g_table = torch.zeros_like(c.table) if (self.chain or self.mappers) else None

    def wants(self, p):
        return p is not None and id(p) in self.want

    def conv(self, layer, g, a, hw, q_rows=0):
        """A convolution ``layer`` whose output has the gradient g and whose input was a() (built only if the weight is asked for)."""
        if self.wants(layer.weight):
            ks = layer.weight.shape[2]
            self.grads[id(layer.weight)] = uo.conv2d_wgrad(g, a(), self.c.B, hw[0], hw[1], ks, q_rows=q_rows, bf16=self.bf16)
        if self.wants(layer.bias):
            self.grads[id(layer.bias)] = uo.bias_grad(g, q_cols=q_rows)

    def norm(self, norm, x, stats, g_y, gelu):
        """An AdaGN whose output (behind the GELU, with ``gelu``) has the gradient g_y: its (w, b) gradient into the table."""
        if self.chain or self.wants(norm.mapper.weight) or self.wants(norm.mapper.bias):
            off = self.c.consts.offsets[norm]
            uo.adagn_wb_grad(x, stats, uv._wb(self.c, norm), g_y, gelu=gelu, out=self.g_table[:, off:off + 2 * norm.c_out])


def _cond_chain(model, c, keep, sink):
    """The conditioning chain in reverse from the gradient table: the mappers, ``mapping`` and ``mapping_cond``."""
    if sink.g_table is None:
        return
    gt, offsets = sink.g_table, c.consts.offsets
    if any(sink.wants(m.mapper.weight) for m in offsets):
        gw = _wgrad(gt, keep.h2, bf16=sink.bf16)                                        # [sum of 2 C, feats]: every mapper's rows at its offset
        for m, off in offsets.items():
            if sink.wants(m.mapper.weight):
                sink.grads[id(m.mapper.weight)] = gw[off:off + 2 * m.c_out]
    if any(sink.wants(m.mapper.bias) for m in offsets):
        gb = ops.colsum(gt).reshape(-1)
        for m, off in offsets.items():
            if sink.wants(m.mapper.bias):
                sink.grads[id(m.mapper.bias)] = gb[off:off + 2 * m.c_out]
    if not sink.chain:
        return
    tc = _train_consts(model, c.consts)
    # g_table map_w, the gradient of mapping's output: the sum runs over ALL mappers' columns (tens of thousands at the CIFAR-shaped model), which
    # the few-rows kernel would walk once per sample; read as a sum over ROWS of gt^T and map_w it is the weight-gradient GEMM's shape
    # (a DATA gradient in the weight-gradient kernel's clothes: it stays split3 under set_wgrad_arithmetic("bf16"))
    g = _wgrad(gt.t().contiguous(), c.consts.map_w)
    for lin, w_t, x_in, has_more in ((model.mapping[2], tc.m2_t, keep.h1, True), (model.mapping[0], tc.m0_t, keep.e, hasattr(model, "mapping_cond"))):
        pre = uo.cond_mlp(x_in, lin.weight, lin.bias)                   # the pre-activation of this layer, recomputed
        g = uo.gelu_vjp(pre, g, out=g)
        if sink.wants(lin.weight):
            sink.grads[id(lin.weight)] = _wgrad(g, x_in, bf16=sink.bf16)
        if sink.wants(lin.bias):
            sink.grads[id(lin.bias)] = ops.colsum(g).reshape(-1)
        if has_more:
            g = uo.cond_mlp(g, w_t)
    if hasattr(model, "mapping_cond") and sink.wants(model.mapping_cond.weight):
        sink.grads[id(model.mapping_cond.weight)] = _wgrad(g, keep.mc, bf16=sink.bf16)


def make_drop(model, key, B, consts):
    """What the walks of models/unet_vjp.py take as ``drop`` for the loss call whose key (one int64 on the device) is ``key``: the key, the
    rate, ``chan`` {residual block: (m1, m2)} -- the blocks' column ranges [B, C] of the table of channel factors, filled here in one launch --
    and ``attn`` {attention layer: site id}."""
    sites = v1.dropout_sites(model)
    chan_sites = [(site, chan) for site, _, kind, chan in sites if kind != "attn"]
    layout, _ = uo.chan_layout(chan_sites)
    if getattr(consts, "drop_sites", None) is None:                     # the (site, offset, C) triples on this device: no copy per call
        consts.drop_sites = torch.tensor(layout, dtype=torch.int64, device=key.device)
    p = float(model.dropout_rate)
    table = uo.chan_mask(key, layout, B, p, sites_dev=consts.drop_sites)
    cols = {site: table[:, off:off + chan] for site, off, chan in layout}
    chan, attn = {}, {}
    for site, layer, kind, _ in sites:
        if kind == "attn":
            attn[layer] = site
        elif kind == "conv1":
            chan[layer] = (cols[site], cols[site + 1])
    return SimpleNamespace(key=key, p=p, table=table, chan=chan, attn=attn)


def primal(model, x, sigma, mapping_cond, drop=None):
    """(F(x, sigma), state): the forward on tensors of this call, and what the backward needs of it.  ``drop``: the loss call's dropout key
    (one int64 on the device; ``loss_forward`` draws it), None without dropout."""
    with torch.no_grad():
        x = x.contiguous()
        B, _, H, W = x.shape
        sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        sizes = v1.level_sizes(model, H, W)
        fingerprint = model._weights_fingerprint()
        consts = uv._consts(model, fingerprint, x.device)
        feats = model.feats_in
        ws = SimpleNamespace(map_w=consts.map_w, map_b=consts.map_b, table=uv._empty(x, B, consts.map_w.shape[0]),
                             **{name: uv._empty(x, B, feats) for name in ("ff", "e", "h1", "h2")})
        c = SimpleNamespace(B=B, consts=consts, table=model._cond_table(sigma, mapping_cond, B, x.device, ws))
        mc = None if mapping_cond is None else mapping_cond.to(device=x.device, dtype=torch.float32).contiguous()
        keep = SimpleNamespace(e=ws.ff if mc is None else ws.e, h1=ws.h1, h2=ws.h2, mc=mc)
        t0 = uo.unet_in(x, model.proj_in.weight, model.proj_in.bias)
        drop = None if drop is None else make_drop(model, drop, B, consts)
        last, tape = uv._primal(model, c, t0, sizes, drop)
        out = uo.unet_out(last, model.proj_out.weight, model.proj_out.bias, tuple(x.shape))
    return out, SimpleNamespace(c=c, keep=keep, tape=tape, last=last, sizes=sizes, fingerprint=fingerprint, x=x, drop=drop)


def backward(model, state, grad_out, want):
    """{id(parameter): gradient} of the parameters ``want`` from the gradient on the primal's output."""
    if model._weights_fingerprint() != state.fingerprint:
        raise RuntimeError("image_v1: the model's weights changed between Denoiser.loss and backward() (its weights fingerprint moved), and the "
                           "backward recomputes from them; compute the loss again")
    with torch.no_grad():
        c, x = state.c, state.x
        B, c_img, H, W = x.shape
        go = grad_out.detach().to(torch.float32).contiguous()
        sink = _Sink(model, c, want)
        geom = (H, W, 1, 1, c_img)
        if sink.wants(model.proj_out.weight):
            sink.grads[id(model.proj_out.weight)] = _wgrad(go, state.last, bf16=sink.bf16, gather=("g", ops.nat.WG_PATCH_NCHW), gather_geom=geom).view_as(
                model.proj_out.weight)
        if sink.wants(model.proj_out.bias):
            sink.grads[id(model.proj_out.bias)] = uo.bias_grad(go)
        g = uo.unet_in(go, c.consts.out_t)                               # proj_out^T: NCHW -> tokens
        g = uv._reverse(model, c, state.tape, g, state.sizes, sink, state.drop)
        if sink.wants(model.proj_in.weight):
            sink.grads[id(model.proj_in.weight)] = _wgrad(g, x, bf16=sink.bf16, gather=("a", ops.nat.WG_PATCH_NCHW), gather_geom=geom).view_as(
                model.proj_in.weight)
        if sink.wants(model.proj_in.bias):
            sink.grads[id(model.proj_in.bias)] = uo.bias_grad(g)
        _cond_chain(model, c, state.keep, sink)
    return sink.grads


class _ParamGrad(torch.autograd.Function):
    """The inner model as an autograd node whose differentiable inputs are its parameters (``Denoiser.loss`` only), after ``_ParamGrad`` of
    models/image_transformer_v2.py.  Forward: ``primal``; kept: its tape and the call's dropout key.  Backward: ``backward`` with the
    parameters autograd asks for."""

    @staticmethod
    def forward(ctx, x, model, sigma, mapping_cond, key, *params):
        out, state = primal(model, x, sigma, mapping_cond, key)
        ctx.model, ctx.params, ctx.state = model, params, state
        ctx.inputs = (x, sigma, mapping_cond, key)                     # the dropout key with them: a recomputation draws the same masks
        return out

    @staticmethod
    def backward(ctx, grad):
        state = ctx.state
        if state is None:                                               # a second backward through a retained graph: the tape is gone
            _, state = primal(ctx.model, *ctx.inputs)
        ctx.state = None
        need = ctx.needs_input_grad[5:]
        want = [p for p, n in zip(ctx.params, need) if n]
        grads = backward(ctx.model, state, grad, want)
        return (None,) * 5 + tuple(grads.get(id(p)) if n else None for p, n in zip(ctx.params, need))


def loss_forward(model, x, sigma, mapping_cond=None, **kwargs):
    """F(x, sigma) of ``model`` (an ``ImageDenoiserModelV1``) for ``Denoiser.loss``: see the module docstring."""
    model._refuse_loss(x, sigma, mapping_cond, **kwargs)
    key = None
    if model._dropout_on and model._dropout_applies():                 # one key per call, drawn on the device: the host does not sync
        key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=x.device, generator=model._dropout_gen)
    params = [p for p in model.parameters() if p.requires_grad] if torch.is_grad_enabled() else []
    if params:
        return _ParamGrad.apply(x, model, sigma, mapping_cond, key, *params)
    return primal(model, x, sigma, mapping_cond, key)[0]

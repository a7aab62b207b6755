"""The reference's U-Net denoiser (k_diffusion/models/image_v1.py: ``ImageDenoiserModelV1``) for SAMPLING on the HIP kernels of
csrc/conv_x3.hip and csrc/unet_f32.hip (wrappers: ``unet_ops``).

The module tree below exists to carry the reference's parameters under the reference's names -- ``state_dict()`` has its keys and shapes,
so a k-diffusion checkpoint loads as it is -- and no sub-module's ``forward`` is ever called.  The model's forward is a fixed list of
kernel launches over fp32 NHWC token buffers ``[B H W, C]``, built once per (batch, height, width):

* a 3 x 3 / 1 x 1 convolution is one ``kd_conv2d_x3`` launch (bias, residual and the output's row stride in its epilogue) -- after
  ``set_conv_arithmetic("bf16")`` one ``kd_conv2d_bf16`` launch (csrc/conv_bf16.hip: bf16 operands, fp32 accumulation), in this list only;
* AdaGN (+ the GELU behind it) is a statistics pass and an apply pass; the (weight, bias) pairs of ALL AdaGN mappers come from one
  ``kd_cond_mlp_f32`` launch over the mappers' concatenated weight;
* ``torch.cat([x, skip], 1)`` is two column ranges of one buffer which their producers write through the row stride;
* self-attention is ``ops.attn_global`` on the qkv convolution's output as it stands; SDPA's scale 1 / 8 (heads of 64) is folded into the q
  rows of the packed qkv weight and bias, which is exact;
* with ``forward_preconditioned`` the Karras scalings ride in ``proj_in`` / ``proj_out``;
* ``forward_jvp`` (the dual pass of ``likelihood.log_likelihood``) is the same walk over buffers of 2 B samples, the tangent stacked behind the
  primal: the linear kernels run once over both, a stacked convolution gives its bias to the primal samples only
  (``kd_conv2d_x3_stacked``), AdaGN has dual kernels (``kd_groupnorm_stats_jvp_f32``, ``kd_adagn_apply_jvp_f32``) and attention is
  ``ops.attn_global_jvp``.  Its primal output has the forward's bits.
* ``forward_vjp`` (gradient guidance: the gradient of a loss on the output w.r.t. the input) returns the output with the forward's bits and a
  pullback; the reverse walk and its recomputation are ``models/unet_vjp.py``, its AdaGN and resampling rules ``csrc/unet_vjp_f32.hip``.

* ``loss_forward`` (what ``Denoiser.loss`` calls: TRAINING) is the one pass behind autograd: a node whose differentiable inputs are the
  parameters; its backward is the reverse walk with the parameter-gradient kernels of csrc/conv_wgrad_x3.hip and csrc/unet_train_f32.hip
  (``models/unet_train.py``); ``set_wgrad_arithmetic("bf16")`` moves the weight-gradient products, and nothing else, to bf16 operands
  (csrc/conv_wgrad_bf16.hip, ``ops.wgrad(bf16=True)``: train.py's ``--mixed-precision bf16``).  In training mode with ``dropout_rate > 0`` it applies the reference's dropout once ``enable_dropout()`` was
  called: Dropout2d behind both convolutions of a residual block (whole (sample, channel) maps, in the convolutions' epilogues) and dropout on
  the attention probabilities, on masks of the project's counter-based generator regenerated wherever they are needed, never stored
  (``dropout_sites``; include/kdiff_unet_drop.h).

Scope: the forward pass, its forward-mode derivative, its reverse-mode derivative w.r.t. the input (explicit methods: ``forward_jvp``,
``forward_vjp``) and the parameter gradients of the training loss (``loss_forward``; sigma and the conditioning get no gradient anywhere) in
fp32-grade (split-bf16x3) arithmetic whatever ``KDIFF_GEMM`` says (the weight-gradient products in bf16 after
``set_wgrad_arithmetic("bf16")``, the sampling forward's convolution products in bf16 after ``set_conv_arithmetic("bf16")``), ``patch_size == 1``, ``skip_stages == 0``, no variance output, no cross
attention, no ``unet_cond``, dropout in ``loss_forward`` only and only after ``enable_dropout()`` (otherwise training mode with
``dropout_rate > 0`` is refused; ``model.eval()`` is always the dropout-free objective), channels that are multiples of 64, even H and W at
every downsample.  Anything else is refused in the constructor; the sampling passes (``forward``, ``forward_jvp``, ``forward_vjp``) raise
NotImplementedError under grad mode with something that requires grad.
"""
from functools import partial

import torch
from torch import nn

from .. import ops
from .. import unet_ops as uo
from .. import weights
from ..augmentation import KarrasAugmentWrapper

_LINEAR = [1 / 8, 3 / 8, 3 / 8, 1 / 8]
MAX_PLANS = 8      # cached launch plans (one per batch / size / device) per model: least recently used beyond that


class _AdaGN(nn.Module):
    """layers.py:162-175 (parameters only)."""

    def __init__(self, feats_in, c_out, num_groups, eps=1e-5):
        super().__init__()
        self.num_groups, self.eps, self.c_out = num_groups, eps, c_out
        self.mapper = nn.Linear(feats_in, c_out * 2)
        nn.init.zeros_(self.mapper.weight)
        nn.init.zeros_(self.mapper.bias)


class _Resample(nn.Module):
    """layers.py:251-280 (the 'linear' kernel buffer only; the kernels carry its values)."""

    def __init__(self, up):
        super().__init__()
        k = torch.tensor([_LINEAR]) * (2 if up else 1)
        self.up = up
        self.register_buffer('kernel', k.T @ k)


class _ResConvBlock(nn.Module):
    """image_v1.py:15-29."""

    def __init__(self, feats_in, c_in, c_mid, c_out, group_size=32, dropout_rate=0.):
        super().__init__()
        self.c_in, self.c_mid, self.c_out = c_in, c_mid, c_out
        self.main = nn.Sequential(
            _AdaGN(feats_in, c_in, max(1, c_in // group_size)), nn.GELU(), nn.Conv2d(c_in, c_mid, 3, padding=1),
            nn.Dropout2d(dropout_rate, inplace=True),
            _AdaGN(feats_in, c_mid, max(1, c_mid // group_size)), nn.GELU(), nn.Conv2d(c_mid, c_out, 3, padding=1),
            nn.Dropout2d(dropout_rate, inplace=True))
        if c_in == c_out:
            self.skip = nn.Identity()
        else:
            self.skip = nn.Conv2d(c_in, c_out, 1, bias=False)
            nn.init.orthogonal_(self.skip.weight)
        nn.init.zeros_(self.main[-2].weight)
        nn.init.zeros_(self.main[-2].bias)


class _SelfAttention2d(nn.Module):
    """layers.py:181-200."""

    def __init__(self, feats_in, c_in, n_head, num_groups, dropout_rate=0.):
        super().__init__()
        self.c_in = self.c_out = c_in
        self.n_head = n_head
        self.norm_in = _AdaGN(feats_in, c_in, num_groups)
        self.qkv_proj = nn.Conv2d(c_in, c_in * 3, 1)
        self.out_proj = nn.Conv2d(c_in, c_in, 1)
        self.dropout = nn.Dropout(dropout_rate)
        nn.init.zeros_(self.out_proj.weight)
        nn.init.zeros_(self.out_proj.bias)


def _block_layers(n_layers, feats_in, c_in, c_mid, c_out, self_attn, dropout_rate, group_size=32, head_size=64):
    mods = []
    for i in range(n_layers):
        my_c_in = c_in if i == 0 else c_mid
        my_c_out = c_mid if i < n_layers - 1 else c_out
        mods.append(_ResConvBlock(feats_in, my_c_in, c_mid, my_c_out, group_size, dropout_rate))
        if self_attn:
            mods.append(_SelfAttention2d(feats_in, my_c_out, max(1, my_c_out // head_size), max(1, my_c_out // group_size), dropout_rate))
    return mods


class _UNet(nn.Module):
    def __init__(self, d_blocks, u_blocks):
        super().__init__()
        self.d_blocks = nn.ModuleList(d_blocks)
        self.u_blocks = nn.ModuleList(u_blocks)
        self.skip_stages = 0


class _MappingNet(nn.Sequential):
    """image_v1.py:80-86."""

    def __init__(self, feats_in, feats_out, n_layers=2):
        mods = []
        for i in range(n_layers):
            lin = nn.Linear(feats_in if i == 0 else feats_out, feats_out)
            nn.init.orthogonal_(lin.weight)
            mods += [lin, nn.GELU()]
        super().__init__(*mods)


def level_sizes(model, H, W):
    """(H, W) of every level of an H x W input; refuses a size that some downsample cannot halve."""
    n = len(model.depths)
    sizes = [(H >> i, W >> i) for i in range(n)]
    for i in range(n - 1):
        if sizes[i][0] % 2 or sizes[i][1] % 2 or min(sizes[i]) < 2:
            raise ValueError(f"image_v1: input size {H}x{W}: level {i} is {sizes[i][0]}x{sizes[i][1]}, which the downsample cannot halve")
    return sizes


DROPOUT_SITE = 1 << 62 | 1 << 33      # the bits every dropout site id of this family carries (include/kdiff_unet_drop.h, mask contract)


def forward_layers(model):
    """The residual blocks and attention layers of ``model`` in the order the forward walks them (the order of ``unet_vjp._primal``'s tape)."""
    out = []
    for block in model.u_net.d_blocks:
        out += list(block)[1:]
    for block in model.u_net.u_blocks:
        out += list(block)[:-1]
    return out


def dropout_sites(model):
    """The dropout sites of ``model`` (an ``ImageDenoiserModelV1``) in forward order: (site id, layer, kind, C).  The layer at position L of
    ``forward_layers(model)``: a residual block has "conv1" = 2^62 | 2^33 | 2 L (Dropout2d behind its first convolution, C = c_mid) and "conv2" =
    2^62 | 2^33 | (2 L + 1) (behind its second, C = c_out), an attention layer "attn" = 2^62 | 2^33 | 2 L (the softmax probabilities, C = c_in).
    Bit 62 set, bit 63 clear, bit 33 set: disjoint from ``image_transformer_v2.dropout_sites``' ids under one key."""
    out = []
    for L, layer in enumerate(forward_layers(model)):
        if isinstance(layer, _ResConvBlock):
            out.append((DROPOUT_SITE | 2 * L, layer, "conv1", layer.c_mid))
            out.append((DROPOUT_SITE | (2 * L + 1), layer, "conv2", layer.c_out))
        else:
            out.append((DROPOUT_SITE | 2 * L, layer, "attn", layer.c_in))
    return out


class _Plan:
    """Buffers and the fixed launch list of one (batch, H, W): ``head`` / ``tail`` take the call's own tensors, ``calls`` is everything between.

    ``dual``: the list of the dual (primal + tangent) pass.  Every activation buffer holds ``S = 2 B`` samples, the primal's rows first and the
    tangent's after (``lo`` / ``hi``), and the linear kernels -- convolutions, resampling -- run once over all of them: they treat samples
    independently.  Only the bias (primal samples alone), AdaGN (its dual kernels) and attention (``ops.attn_global_jvp`` on the two halves)
    tell the halves apart."""

    def __init__(self, model, B, H, W, device, dual=False):
        n, ch = len(model.depths), model.channels
        sizes = level_sizes(model, H, W)
        f32 = dict(device=device, dtype=torch.float32)
        feats = model.feats_in
        self.B, self.calls, pool = B, [], {}
        S = 2 * B if dual else B                                        # samples in every activation buffer
        bias_batch = B if dual else None

        def lo(t):
            return t[:t.shape[0] // 2]

        def hi(t):
            return t[t.shape[0] // 2:]
        self.ff, self.e, self.h1, self.h2 = (torch.empty(B, feats, **f32) for _ in range(4))

        def alloc(rows, cols):
            free_list = pool.get((rows, cols))
            return free_list.pop() if free_list else torch.empty(rows, cols, **f32)

        def free(t):
            if t.is_contiguous() and t.storage_offset() == 0:          # (a column range of a concat buffer is not the pool's)
                pool.setdefault(tuple(t.shape), []).append(t)

        # every AdaGN mapper in one weight: its (weight, bias) pair is a column range of the table
        norms = [m for m in model.u_net.modules() if isinstance(m, _AdaGN)]
        self.map_w = torch.cat([m.mapper.weight.detach() for m in norms]).contiguous()
        self.map_b = torch.cat([m.mapper.bias.detach() for m in norms]).contiguous()
        self.table = torch.empty(B, self.map_w.shape[0], **f32)
        offsets, off = {}, 0
        for m in norms:
            offsets[m] = off
            off += 2 * m.c_out
        emit = self.calls.append

        def adagn(norm, x, out, gelu):
            stats = torch.empty(B, norm.num_groups, 4, **f32)
            wb = self.table[:, offsets[norm]:offsets[norm] + 2 * norm.c_out]
            if dual:
                jstats = torch.empty_like(stats)
                emit(partial(uo.groupnorm_stats_jvp, lo(x), hi(x), B, norm.num_groups, norm.eps, out=stats, out_dot=jstats))
                emit(partial(uo.adagn_apply_jvp, lo(x), hi(x), stats, jstats, wb, gelu=gelu, out=lo(out), out_dot=hi(out)))
                return
            emit(partial(uo.groupnorm_stats, x, B, norm.num_groups, norm.eps, out=stats))
            emit(partial(uo.adagn_apply, x, stats, wb, gelu=gelu, out=out))

        # set_conv_arithmetic("bf16"): every convolution of the SAMPLING list on kd_conv2d_bf16; the dual list keeps the fp32-grade kernel
        arithmetic = {"bf16": True} if model.conv_arithmetic == "bf16" and not dual else {}

        def conv(x, weight, hw, bias=None, residual=None, out=None, packed=None):
            emit(partial(uo.conv2d, x, weight, S, hw[0], hw[1], bias=bias, residual=residual, out=out,
                         packed=uo.pack_conv(weight) if packed is None else packed, bias_batch=None if bias is None else bias_batch, **arithmetic))

        def res_block(layer, x, y, hw):
            rows = x.shape[0]
            t1 = alloc(rows, layer.c_in)
            adagn(layer.main[0], x, t1, True)
            t2 = alloc(rows, layer.c_mid)
            conv(t1, layer.main[2].weight, hw, bias=layer.main[2].bias, out=t2)
            free(t1)
            adagn(layer.main[4], t2, t2, True)
            res = x
            if isinstance(layer.skip, nn.Conv2d):
                res = alloc(rows, layer.c_out)
                conv(x, layer.skip.weight, hw, out=res)
            conv(t2, layer.main[6].weight, hw, bias=layer.main[6].bias, residual=res, out=y)
            free(t2)
            if res is not x:
                free(res)

        def attention(layer, x, y, hw):
            rows, C = x.shape[0], layer.c_in
            t1 = alloc(rows, C)
            adagn(layer.norm_in, x, t1, False)
            # SDPA scales q k^T by 1 / sqrt(64): a power of two, folded into the q rows (the first C output channels) exactly
            wq, bq = layer.qkv_proj.weight.detach().clone(), layer.qkv_proj.bias.detach().clone()
            wq[:C] *= 0.125
            bq[:C] *= 0.125
            qkv = alloc(rows, 3 * C)
            conv(t1, wq, hw, bias=bq, out=qkv, packed=uo.pack_conv(wq, cache=False))
            free(t1)
            a = alloc(rows, C)
            q3, a3 = qkv.view(S, hw[0] * hw[1], 3 * C), a.view(S, hw[0] * hw[1], C)
            if dual:
                # the tangent from the fp32 dual kernel; its primal output is then overwritten by the forward's own kernel, so that the dual
                # pass's primal has the forward's bits
                emit(partial(ops.attn_global_jvp, q3[:B], q3[B:], layer.n_head, out=a3[:B], out_dot=a3[B:]))
                q3, a3 = q3[:B], a3[:B]
            emit(partial(ops.attn_global, q3, layer.n_head, out=a3))
            free(qkv)
            conv(a, layer.out_proj.weight, hw, bias=layer.out_proj.bias, residual=x, out=y)
            free(a)

        def run_layer(layer, x, y, hw):
            (res_block if isinstance(layer, _ResConvBlock) else attention)(layer, x, y, hw)

        self.t0 = cur = alloc(S * H * W, ch[0])
        cats = [None] * n
        for i, block in enumerate(model.u_net.d_blocks):
            hw = sizes[i]
            rows = S * hw[0] * hw[1]
            if i > 0:
                nxt = alloc(rows, ch[i - 1])
                emit(partial(uo.down2, cur, S, sizes[i - 1][0], sizes[i - 1][1], out=nxt))
                cur = nxt
            layers = list(block)[1:]
            for j, layer in enumerate(layers):
                if j == len(layers) - 1 and i < n - 1:                  # the level's skip: the right half of the up path's concat buffer
                    cats[i] = alloc(rows, 2 * ch[i])
                    dst = cats[i][:, ch[i]:]
                else:
                    dst = alloc(rows, layer.c_out)
                run_layer(layer, cur, dst, hw)
                free(cur)
                cur = dst
        for k, block in enumerate(model.u_net.u_blocks):
            i = n - 1 - k
            hw = sizes[i]
            rows = S * hw[0] * hw[1]
            if i < n - 1:
                cur = cats[i]                                           # [upsampled | skip], both halves written by now
            for layer in list(block)[:-1]:
                dst = alloc(rows, layer.c_out)
                run_layer(layer, cur, dst, hw)
                free(cur)
                cur = dst
            if i > 0:
                emit(partial(uo.up2, cur, S, hw[0], hw[1], out=cats[i - 1][:, :ch[i - 1]]))
                free(cur)
        self.last = cur


class AugmentWrapperV1(KarrasAugmentWrapper):
    """``KarrasAugmentWrapper`` around the U-Net (config.py:169-170) that also hands ``Denoiser.forward`` the inner model's fused
    ``forward_preconditioned`` -- and ``Denoiser.forward_jvp`` / ``forward_vjp`` its ``forward_jvp`` / ``forward_vjp`` -- with the same
    conditioning rule: ``aug_cond`` (zeros [B, 9] when none is given) in front of ``mapping_cond``."""

    def forward_preconditioned(self, input, sigma, sigma_data, aug_cond=None, mapping_cond=None, **kwargs):
        cond = input.new_zeros([input.shape[0], 9]) if aug_cond is None else aug_cond
        if mapping_cond is not None:
            cond = torch.cat([cond, mapping_cond], dim=1)
        return self.inner_model.forward_preconditioned(input, sigma, sigma_data, mapping_cond=cond, **kwargs)

    def forward_jvp(self, input, sigma, tangent, sigma_data=None, aug_cond=None, mapping_cond=None, **kwargs):
        """The inner model's ``forward_jvp`` under the conditioning rule of ``forward_preconditioned``."""
        cond = input.new_zeros([input.shape[0], 9]) if aug_cond is None else aug_cond
        if mapping_cond is not None:
            cond = torch.cat([cond, mapping_cond], dim=1)
        return self.inner_model.forward_jvp(input, sigma, tangent, mapping_cond=cond, sigma_data=sigma_data, **kwargs)


    def forward_vjp(self, input, sigma, sigma_data=None, aug_cond=None, mapping_cond=None, **kwargs):
        """The inner model's ``forward_vjp`` under the conditioning rule of ``forward_preconditioned``."""
        cond = input.new_zeros([input.shape[0], 9]) if aug_cond is None else aug_cond
        if mapping_cond is not None:
            cond = torch.cat([cond, mapping_cond], dim=1)
        return self.inner_model.forward_vjp(input, sigma, mapping_cond=cond, sigma_data=sigma_data, **kwargs)

    def loss_forward(self, input, sigma, aug_cond=None, mapping_cond=None, **kwargs):
        """The inner model's ``loss_forward`` (``Denoiser.loss``) under the conditioning rule of ``forward_preconditioned``."""
        cond = input.new_zeros([input.shape[0], 9]) if aug_cond is None else aug_cond
        if mapping_cond is not None:
            cond = torch.cat([cond, mapping_cond], dim=1)
        return self.inner_model.loss_forward(input, sigma, mapping_cond=cond, **kwargs)


class ImageDenoiserModelV1(nn.Module):
    """image_v1.py:89-176 with the reference's constructor signature, attributes, state_dict and ``param_groups``; the forward, its
    forward-mode derivative and its input gradient as explicit methods; behind autograd only ``loss_forward``, the training loss's parameter
    gradients (see the module docstring for the scope)."""

    def __init__(self, c_in, feats_in, depths, channels, self_attn_depths, cross_attn_depths=None, mapping_cond_dim=0, unet_cond_dim=0,
                 cross_cond_dim=0, dropout_rate=0., patch_size=1, skip_stages=0, has_variance=False):
        super().__init__()
        for field, value, want in (("patch_size", patch_size, 1), ("skip_stages", skip_stages, 0), ("has_variance", bool(has_variance), False),
                                   ("cross_cond_dim", cross_cond_dim, 0), ("unet_cond_dim", unet_cond_dim, 0)):
            if value != want:
                raise ValueError(f"image_v1: {field}={value!r} is not supported on the HIP path (only {field}={want!r})")
        if mapping_cond_dim < 0:
            raise ValueError(f"image_v1: mapping_cond_dim={mapping_cond_dim} must be >= 0")
        depths, channels, self_attn_depths = list(depths), list(channels), list(self_attn_depths)
        if not depths or not (len(depths) == len(channels) == len(self_attn_depths)):
            raise ValueError(f"image_v1: depths, channels and self_attn_depths must have one entry per level (got {len(depths)}, {len(channels)}, "
                             f"{len(self_attn_depths)})")
        if any(c <= 0 or c % 64 for c in channels):
            raise ValueError(f"image_v1: channels={channels}: every channel count must be a multiple of 64 (heads of 64, groups of 32)")
        if any(d < 1 for d in depths):
            raise ValueError(f"image_v1: depths={depths}: every level needs at least one block")
        if not 1 <= c_in <= 4:
            raise ValueError(f"image_v1: c_in={c_in}: 1 to 4 image channels")
        if feats_in <= 0 or feats_in % 2:
            raise ValueError(f"image_v1: feats_in={feats_in} must be even and positive")
        self.c_in, self.feats_in, self.depths, self.channels = c_in, feats_in, depths, channels
        self.unet_cond_dim, self.patch_size, self.has_variance, self.dropout_rate = unet_cond_dim, patch_size, has_variance, dropout_rate
        from ..layers import FourierFeatures
        self.timestep_embed = FourierFeatures(1, feats_in)
        if mapping_cond_dim > 0:
            self.mapping_cond = nn.Linear(mapping_cond_dim, feats_in, bias=False)
        self.mapping = _MappingNet(feats_in, feats_in)
        self.proj_in = nn.Conv2d(c_in, channels[0], 1)
        self.proj_out = nn.Conv2d(channels[0], c_in, 1)
        nn.init.zeros_(self.proj_out.weight)
        nn.init.zeros_(self.proj_out.bias)
        n = len(depths)
        d_blocks, u_blocks = [], []
        for i in range(n):
            mods = _block_layers(depths[i], feats_in, channels[max(0, i - 1)], channels[i], channels[i], self_attn_depths[i], dropout_rate)
            d_blocks.append(nn.Sequential(_Resample(False) if i > 0 else nn.Identity(), *mods))
        for i in range(n):
            my_c_in = channels[i] * 2 if i < n - 1 else channels[i]
            mods = _block_layers(depths[i], feats_in, my_c_in, channels[i], channels[max(0, i - 1)], self_attn_depths[i], dropout_rate)
            u_blocks.append(nn.Sequential(*mods, _Resample(True) if i > 0 else nn.Identity()))
        self.u_net = _UNet(d_blocks, reversed(u_blocks))
        self._watch, self._plan_cache, self._fingerprint = weights.WeightWatch(self), weights.PlanCache(), None
        self._plans = self._plan_cache.plans
        self._dual_cache = weights.PlanCache()         # the dual pass's plans: forward_jvp leaves ``_plans`` and its eviction order alone
        self._vjp_cache, self._vjp_fingerprint = weights.PlanCache(), None       # forward_vjp's weight-derived tensors (models/unet_vjp.py)
        self._dropout_on, self._dropout_gen = False, None                        # enable_dropout(): not part of the state_dict
        self.wgrad_arithmetic = None                                             # set_wgrad_arithmetic(): not part of the state_dict
        self.conv_arithmetic = None                                              # set_conv_arithmetic(): not part of the state_dict

    def param_groups(self, base_lr=2e-4):
        """image_v1.py:117-133: the weights of ``mapping`` and ``u_net`` decay, everything else does not."""
        wd, no_wd = [], []
        for name, param in self.named_parameters():
            (wd if (name.startswith("mapping") or name.startswith("u_net")) and name.endswith(".weight") else no_wd).append(param)
        return [{"params": wd, "lr": base_lr}, {"params": no_wd, "lr": base_lr, "weight_decay": 0.0}]

    def set_skip_stages(self, skip_stages):
        if skip_stages != 0:
            raise ValueError(f"image_v1: skip_stages={skip_stages!r} is not supported on the HIP path (only skip_stages=0)")
        return self

    def set_patch_size(self, patch_size):
        if patch_size != 1:
            raise ValueError(f"image_v1: patch_size={patch_size!r} is not supported on the HIP path (only patch_size=1)")

    def enable_dropout(self, generator=None):
        """Opt in to dropout in the training loss: from now on ``loss_forward`` (``Denoiser.loss``) of the model in training mode applies
        ``dropout_rate`` at the reference's sites (``dropout_sites``), on masks of this project's counter-based generator
        (include/kdiff_unet_drop.h, mask contract) -- not torch's dropout RNG stream.  Each such call draws one int64 key on the device from
        ``generator`` (a torch.Generator on the model's device; None: the default generator of the input's device, so torch.manual_seed
        governs it) without a host sync; the backward pass regenerates the same masks from it.  The sampling passes (``forward``,
        ``forward_jvp``, ``forward_vjp``) have no dropout and keep refusing training mode with a rate: call model.eval() for them, which is
        always the dropout-free objective.  The setting is not part of the state_dict.  Returns the model."""
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError(f"ImageDenoiserModelV1.enable_dropout: dropout_rate must lie in [0, 1) (dropout_rate = {self.dropout_rate})")
        if generator is not None and not isinstance(generator, torch.Generator):
            raise TypeError(f"enable_dropout: generator must be a torch.Generator or None (got {type(generator)})")
        self._dropout_on, self._dropout_gen = True, generator
        return self

    def set_wgrad_arithmetic(self, arithmetic=None):
        """Opt in to bf16 weight gradients in the training loss.  ``None`` (the default): split-bf16 x 3, the family's fp32-grade arithmetic.
        ``"bf16"``: every weight-gradient product of ``loss_forward``'s backward -- the convolutions' (``kd_conv2d_wgrad_bf16``,
        include/kdiff_unet_mixed.h, ks = 3 and ks = 1) and the GEMMs of the mappers, ``mapping``, ``mapping_cond``, ``proj_in`` and ``proj_out``
        (``ops.wgrad(bf16=True)``) -- rounds both operands once to bf16 and accumulates in fp32, one MFMA per product: a ``Conv2d`` / ``Linear``
        backward of the reference under ``--mixed-precision bf16``.  Only those products move: the primal (so the loss), the data-gradient
        convolutions, AdaGN and its (w, b) sums, the bias gradients, the attention rules, the way back through the mappers, the dropout masks
        and ``forward_vjp`` keep their arithmetic.  The setting is not part of the state_dict.  Returns the model."""
        if arithmetic not in (None, "bf16"):
            raise ValueError(f"ImageDenoiserModelV1.set_wgrad_arithmetic: {arithmetic!r} (None or 'bf16')")
        self.wgrad_arithmetic = arithmetic
        return self

    def set_conv_arithmetic(self, arithmetic=None):
        """Opt in to bf16 convolutions in the sampling forward.  ``None`` (the default): split-bf16 x 3, the family's fp32-grade arithmetic.
        ``"bf16"``: every convolution of the residual and attention blocks in ``forward`` / ``forward_preconditioned`` rounds its activations
        once to bf16 while staging them, takes the bf16 rounding of its weights and accumulates in fp32, one MFMA per product
        (``kd_conv2d_bf16``, include/kdiff_unet_bf16.h): a ``Conv2d`` of the reference under ``torch.autocast(bfloat16)``.  Only those products
        move: activations stay fp32 in memory, and ``proj_in`` / ``proj_out`` with the preconditioning, AdaGN, the mappers, resampling and
        attention keep their arithmetic -- as do ``forward_jvp`` / ``log_likelihood``, ``forward_vjp`` and ``loss_forward`` with its
        backward, whatever the setting.  A change drops the cached launch plans.  The setting is not part of the state_dict.  Returns the
        model."""
        if arithmetic not in (None, "bf16"):
            raise ValueError(f"ImageDenoiserModelV1.set_conv_arithmetic: {arithmetic!r} (None or 'bf16')")
        if arithmetic != self.conv_arithmetic:
            self.conv_arithmetic = arithmetic
            self._plan_cache.drop_all()
        return self

    def _dropout_rates(self):
        """(name, rate) of every dropout rate of the model: what ``enable_dropout`` serves (train.py's opt-in test, as the transformer's)."""
        return [("dropout_rate", self.dropout_rate)]

    def _dropout_applies(self):
        return bool(self.training and self.dropout_rate)

    # ---- launch plans ---------------------------------------------------------------------------------------------------------------------
    def _weights_fingerprint(self):
        return self._watch.fingerprint()

    def invalidate(self):
        """Drop the launch plans at the next call (needed only after an in-place edit of weights created under torch.inference_mode())."""
        self._watch.bump()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._watch.bump()
        return out

    def _plan(self, B, H, W, device, dual=False):
        fp = self._weights_fingerprint()
        if fp != self._fingerprint:
            self._plan_cache.drop_all()
            self._dual_cache.drop_all()
            self._fingerprint = fp
        key = (B, H, W, str(device))
        cache = self._dual_cache if dual else self._plan_cache
        return cache.get(key) or cache.put(key, lambda: _Plan(self, B, H, W, device, dual), MAX_PLANS)

    def _refuse(self, input, sigma, mapping_cond, unet_cond=None, cross_cond=None, cross_cond_padding=None, return_variance=False, tangent=None,
                dual=False):
        """The refusals of the sampling passes (forward, dual, reverse): what the HIP path does not take, by name."""
        self._refuse_conditioning(unet_cond, cross_cond, cross_cond_padding, return_variance)
        tensors = [t for t in (input, sigma, mapping_cond, tangent) if isinstance(t, torch.Tensor)]
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("image_v1: sampling only -- the U-Net has no backward pass on the HIP path; call it under torch.no_grad() "
                                      "(and model.requires_grad_(False))")
        if self.training and self.dropout_rate:
            raise NotImplementedError("image_v1: sampling only -- dropout is a training quantity; call model.eval()")
        self._check_operands(input, mapping_cond, tangent, dual)

    @staticmethod
    def _refuse_conditioning(unet_cond=None, cross_cond=None, cross_cond_padding=None, return_variance=False):
        if unet_cond is not None or cross_cond is not None or cross_cond_padding is not None or return_variance:
            raise ValueError("image_v1: unet_cond, cross_cond and return_variance are not supported on the HIP path")

    def _refuse_loss(self, input, sigma, mapping_cond, unet_cond=None, cross_cond=None, cross_cond_padding=None, return_variance=False):
        """The refusals of ``loss_forward``: the parameters MAY require grad here; the data may not, and dropout is opt-in."""
        self._refuse_conditioning(unet_cond, cross_cond, cross_cond_padding, return_variance)
        for name, t in (("input", input), ("sigma", sigma), ("mapping_cond", mapping_cond)):
            if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
                raise NotImplementedError(f"image_v1: loss_forward differentiates w.r.t. the parameters only; {name} gets no gradient (pass "
                                          f"{name}.detach(), or use forward_vjp for the input gradient)")
        if self._dropout_applies() and not self._dropout_on:
            raise NotImplementedError(f"image_v1: dropout_rate={self.dropout_rate} in training mode: the U-Net's Dropout2d is not implemented on the "
                                      f"HIP path; call model.eval() for the dropout-free objective (or opt in with model.enable_dropout(): "
                                      f"masks from this project's counter-based generator, in loss_forward only)")
        self._check_operands(input, mapping_cond)

    def _check_operands(self, input, mapping_cond, tangent=None, dual=False):
        """Shapes, devices and dtypes of a call's tensors (every pass)."""
        if not isinstance(input, torch.Tensor) or input.dim() != 4 or input.shape[1] != self.c_in:
            raise ValueError(f"image_v1: input is [B, {self.c_in}, H, W] (got {tuple(getattr(input, 'shape', ()))})")
        if dual and (not isinstance(tangent, torch.Tensor) or tangent.shape != input.shape):
            raise ValueError(f"image_v1: tangent has the input's shape {tuple(input.shape)} (got {tuple(getattr(tangent, 'shape', ()))})")
        if not input.is_cuda:
            raise RuntimeError(f"image_v1 runs on the HIP path only: move the model and inputs to a ROCm device (got {input.device}); there is no "
                               f"CPU fallback")
        if self.proj_in.weight.device != input.device:
            raise RuntimeError(f"model weights are on {self.proj_in.weight.device}, input on {input.device}")
        if input.dtype != torch.float32 or self.proj_in.weight.dtype != torch.float32:
            raise TypeError(f"image_v1: fp32 inputs and weights only (got {input.dtype}, {self.proj_in.weight.dtype})")
        has_cond = hasattr(self, "mapping_cond")
        if mapping_cond is not None and not has_cond:
            raise ValueError("image_v1: mapping_cond given, but the model was built with mapping_cond_dim=0")
        if dual:
            if tangent.device != input.device:
                raise RuntimeError(f"image_v1: tangent is on {tangent.device}, input on {input.device}")
            if tangent.dtype != torch.float32:
                raise TypeError(f"image_v1: tangent is fp32 like the input (got {tangent.dtype})")

    def _cond_table(self, sigma, mapping_cond, B, device, ws):
        """The conditioning of one call: Fourier features of sigma (+ mapping_cond), the mapping network, and every AdaGN mapper's (weight,
        bias) pair into ``ws.table``.  ``ws`` holds the buffers ff, e, h1, h2, table and the concatenated mapper weight map_w / map_b."""
        e = ops.fourier_sigma(sigma, self.timestep_embed.weight, out=ws.ff)
        if mapping_cond is not None:
            mc = mapping_cond.to(device=device, dtype=torch.float32).contiguous()
            if tuple(mc.shape) != (B, self.mapping_cond.weight.shape[1]):
                raise ValueError(f"image_v1: mapping_cond is [{B}, {self.mapping_cond.weight.shape[1]}] (got {tuple(mc.shape)})")
            e = uo.cond_mlp(mc, self.mapping_cond.weight, add=ws.ff, out=ws.e)
        h = uo.cond_mlp(e, self.mapping[0].weight, self.mapping[0].bias, gelu=True, out=ws.h1)
        h = uo.cond_mlp(h, self.mapping[2].weight, self.mapping[2].bias, gelu=True, out=ws.h2)
        return uo.cond_mlp(h, ws.map_w, ws.map_b, out=ws.table)

    def _run(self, input, sigma, mapping_cond, sigma_data, unet_cond=None, cross_cond=None, cross_cond_padding=None, return_variance=False,
             tangent=None, dual=False):
        self._refuse(input, sigma, mapping_cond, unet_cond, cross_cond, cross_cond_padding, return_variance, tangent, dual)
        x = input.contiguous()
        B, _, H, W = x.shape
        sigma = sigma.to(device=x.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        plan = self._plan(B, H, W, x.device, dual)
        self._cond_table(sigma, mapping_cond, B, x.device, plan)
        pre = sigma_data is not None
        scale = dict(sigma=sigma if pre else None, sigma_data=sigma_data if pre else 1.0)
        rows = B * H * W
        t0, last = (plan.t0[:rows], plan.last[:rows]) if dual else (plan.t0, plan.last)
        uo.unet_in(x, self.proj_in.weight, self.proj_in.bias, out=t0, **scale)
        if dual:                                       # the tangent of both projections: no bias, x_dot in the image's place
            x_dot = tangent.contiguous()
            uo.unet_in(x_dot, self.proj_in.weight, None, out=plan.t0[rows:], **scale)
        for call in plan.calls:
            call()
        out = uo.unet_out(last, self.proj_out.weight, self.proj_out.bias, tuple(x.shape), image=x if pre else None, **scale)
        if not dual:
            return out
        return out, uo.unet_out(plan.last[rows:], self.proj_out.weight, None, tuple(x.shape), image=x_dot if pre else None, **scale)

    def forward(self, input, sigma, mapping_cond=None, unet_cond=None, cross_cond=None, cross_cond_padding=None, return_variance=False):
        """F(input, sigma): [B, C, H, W] fp32 on a ROCm device -> [B, C, H, W] (image_v1.py:135-157)."""
        return self._run(input, sigma, mapping_cond, None, unet_cond, cross_cond, cross_cond_padding, return_variance)

    def forward_preconditioned(self, input, sigma, sigma_data, mapping_cond=None, **kwargs):
        """D(x, sigma) = F(x c_in, sigma) c_out + x c_skip (k_diffusion/layers.py:88-90) with c_in folded into ``proj_in`` and c_out / c_skip
        into ``proj_out``: what ``Denoiser.forward`` calls."""
        return self._run(input, sigma, mapping_cond, float(sigma_data), **kwargs)

    def forward_jvp(self, input, sigma, tangent, mapping_cond=None, sigma_data=None, **kwargs):
        """(out, out_dot): F(input, sigma) -- or D(input, sigma) with ``sigma_data``, the scalings folded in as in ``forward_preconditioned`` --
        and its forward-mode derivative along ``tangent``, sigma and the conditioning held fixed: what ``Denoiser.forward_jvp`` and
        ``likelihood.log_likelihood`` call.  One dual pass over [primal | tangent] buffers (``_Plan``); it builds no autograd graph, and the
        refusals are the forward's."""
        return self._run(input, sigma, mapping_cond, None if sigma_data is None else float(sigma_data), tangent=tangent, dual=True, **kwargs)

    def forward_vjp(self, input, sigma, mapping_cond=None, sigma_data=None, **kwargs):
        """(out, pullback) in the shape of ``torch.func.vjp``: out = F(input, sigma) -- or D(input, sigma) with ``sigma_data``, folded in as in
        ``forward_preconditioned`` -- with the forward's bits, and ``pullback(grad_out)`` = J^T grad_out w.r.t. ``input``, sigma, the
        conditioning and the weights held fixed: what ``Denoiser.forward_vjp`` and gradient guidance call.  The pullback may be called more
        than once; it raises if the weights changed since the primal.  The reverse walk is ``models/unet_vjp.py``; it builds no autograd
        graph and touches no launch plan, and the refusals are the forward's."""
        from . import unet_vjp
        return unet_vjp.forward_vjp(self, input, sigma, mapping_cond, sigma_data, **kwargs)

    def loss_forward(self, input, sigma, mapping_cond=None, **kwargs):
        """F(input, sigma) for ``Denoiser.loss`` (which hands it the input already scaled by c_in): the forward's kernels on tensors of this
        call.  Under grad mode the output carries a ``grad_fn`` whose backward fills the ``.grad`` of every parameter that requires grad
        (models/unet_train.py); a parameter that does not costs no launch.  input, sigma and the conditioning get no gradient; training mode
        with ``dropout_rate > 0`` applies the dropout once ``enable_dropout()`` was called (one key drawn per call) and is refused without
        it (``model.eval()`` gives the dropout-free objective).  The sampling passes above keep refusing grad mode: training goes through
        here only."""
        from . import unet_train
        return unet_train.loss_forward(self, input, sigma, mapping_cond, **kwargs)

"""Hourglass diffusion transformer ("image_transformer_v2") denoiser, MI355X-native forward.

Drop-in for ``k_diffusion.models.ImageTransformerDenoiserModelV2``
(k_diffusion/models/image_transformer_v2.py:667-762): same constructor, same ``forward(x, sigma,
aug_cond, class_cond, mapping_cond)``, same ``state_dict`` keys and shapes (the checkpoint
contract), same error behaviour for missing conditioning.

What differs is *how* the forward runs.  The reference is a tree of nn.Modules issuing ~5 400
ATen / Triton / NATTEN / flash-attn launches per forward.  Here the module tree only *holds*
weights; the forward is a flat, pre-planned list of ~90 launches of hand-written gfx950 kernels
(csrc/, C ABI in include/kdiff_hip.h) over a token-major fp32 workspace:

  conditioning : FourierFeatures kernel -> GEMMs (mapping network) -> ONE GEMM producing every
                 AdaRMSNorm scale of the network ([B, sum(d)] table, "+1" folded into the epilogue)
  patch_in     : NCHW gather + patch + Linear (+ Karras c_in) in one GEMM
  each layer   : [AdaRMSNorm -> qkv GEMM] -> attention core with cosine-sim scaling and axial RoPE
                 applied on the fly -> [out_proj GEMM + residual] ;
                 [AdaRMSNorm -> up GEMM -> GEGLU] -> [down GEMM + residual]
  merge/split  : 2x2 space-to-depth / depth-to-space folded into GEMM addressing; lerp in the epilogue
  patch_out    : [RMSNorm -> GEMM -> NHWC->NCHW scatter (+ Karras c_out, c_skip)] in one GEMM

The plan (workspace + prebuilt launch descriptors) is cached per input shape.  There is no eager /
CPU path: calling ``forward`` without a ROCm device or without the built library raises.
"""
import ctypes as C
import os
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Union

import torch
from torch import nn

from .. import _native as nat
from .. import ops
from .. import weights
from . import axial_rope
from .cond_tables import ScaleTables

D_HEAD = 64
DERIVED_KEPT = 1024  # weight-derived tensors kept per model (_derive: transposed weights, RoPE tables, ...): all dropped beyond that
MAX_PLANS = 16     # cached launch plans (one per batch / size / conditioning kinds / device / arithmetic mode / switches) per model: least recently used beyond that
# environment switches of the kernel routing (name, default): read in _plan_for, part of the plan key, passed to route_layer
PLAN_SWITCHES = (("KDIFF_ATTN_BLOCK", "1"), ("KDIFF_PROJ_BLOCK", "1"), ("KDIFF_FFN_OUT", "all"), ("KDIFF_RUN_LIST", "1"), ("KDIFF_ATTN_FFN", "1"))
CLASS_IDS_KEPT = 4            # range-checked class_cond tensors remembered per plan (cond / uncond pairs of a guidance wrapper)


# ---------------------------------------------------------------------------------- configuration

@dataclass
class GlobalAttentionSpec:
    d_head: int


@dataclass
class NeighborhoodAttentionSpec:
    d_head: int
    kernel_size: int


@dataclass
class ShiftedWindowAttentionSpec:
    d_head: int
    window_size: int


@dataclass
class NoAttentionSpec:
    pass


@dataclass
class LevelSpec:
    depth: int
    width: int
    d_ff: int
    self_attn: Union[GlobalAttentionSpec, NeighborhoodAttentionSpec, ShiftedWindowAttentionSpec, NoAttentionSpec]
    dropout: float


@dataclass
class MappingSpec:
    depth: int
    width: int
    d_ff: int
    dropout: float


# ---------------------------------------------------------------------------------- weight holders

class _Holder(nn.Module):
    """Names a group of parameters / sub-holders so that state_dict keys match the reference."""

    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            if isinstance(v, nn.Parameter):
                self.register_parameter(k, v)
            elif isinstance(v, torch.Tensor):
                self.register_buffer(k, v)
            else:
                self.add_module(k, v)


def _linear_weight(out_f, in_f, zero=False):
    """nn.Linear's default init (kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(in), 1/sqrt(in))), or the
    reference's zero_init (image_transformer_v2.py:37-41)."""
    w = torch.zeros(out_f, in_f)
    if not zero:
        bound = 1.0 / math.sqrt(in_f)
        w.uniform_(-bound, bound)
    return _Holder(weight=nn.Parameter(w))


def _layer(spec: LevelSpec, cond_features: int):
    d, parts = spec.width, {}
    if not isinstance(spec.self_attn, NoAttentionSpec):
        nh = d // spec.self_attn.d_head
        parts["self_attn"] = _Holder(
            scale=nn.Parameter(torch.full([nh], 10.0)),
            norm=_Holder(linear=_linear_weight(d, cond_features, zero=True)),
            qkv_proj=_linear_weight(3 * d, d),
            pos_emb=_Holder(freqs=axial_rope.rope_freqs(spec.self_attn.d_head // 2, nh)),
            out_proj=_linear_weight(d, d, zero=True))
    parts["ff"] = _Holder(norm=_Holder(linear=_linear_weight(d, cond_features, zero=True)),
                          up_proj=_linear_weight(2 * spec.d_ff, d),
                          down_proj=_linear_weight(d, spec.d_ff, zero=True))
    return _Holder(**parts)


def _rms_scale(n):
    return _Holder(scale=nn.Parameter(torch.ones(n)))


# ---------------------------------------------------------------------------------- the hourglass's structure (every pass walks it)

_ATTN_KIND = {GlobalAttentionSpec: "global", NeighborhoodAttentionSpec: "neighborhood", ShiftedWindowAttentionSpec: "shifted-window"}
_CORE = {"global": "attn_global", "neighborhood": "attn_na2d", "shifted-window": "attn_window"}


def attn_geometry(spec, index):
    """(kind, core, params) of the attention of layer ``index`` (``Step.index``) of a level with attention ``spec``: ``kind`` as
    route_layer takes it, ``core`` the name of its kernels (ops.<core>, ops.<core>_jvp, ops.<core>_vjp; kd_<core>_f32 / _bf16) and
    ``params`` their arguments behind the head count: () / (kernel_size,) / (window_size, shift)."""
    kind = _ATTN_KIND[type(spec)]
    if kind == "global":
        params = ()
    elif kind == "neighborhood":
        params = (spec.kernel_size,)
    else:
        params = (spec.window_size, spec.window_size // 2 if index % 2 == 1 else 0)          # shift: :523
    return kind, _CORE[kind], params


class Step(NamedTuple):
    """One step of ``hourglass``: kind "layer" (``module`` of level ``level``, state-dict prefix ``prefix``, ``index`` its position in
    the level with the up levels' offset already applied), or "merge" / "split" between levels ``level`` and ``level + 1``."""
    kind: str
    level: int
    prefix: str = ""
    module: Optional[nn.Module] = None
    index: int = 0


def hourglass(model):
    """The network's steps in forward order (image_transformer_v2.py:721-762): down levels, each followed by its merge, the mid level,
    then each up level behind its split.  An up level's layers count on from its down level's (:697), which sets the window shift."""
    steps, top = [], len(model.level_specs) - 1
    for li in range(top):
        steps += [Step("layer", li, f"down_levels.{li}.{i}.", mod, i) for i, mod in enumerate(model.down_levels[li])]
        steps.append(Step("merge", li))
    steps += [Step("layer", top, f"mid_level.{i}.", mod, i) for i, mod in enumerate(model.mid_level)]
    for li in reversed(range(top)):
        steps.append(Step("split", li))
        depth = model.level_specs[li].depth
        steps += [Step("layer", li, f"up_levels.{li}.{i}.", mod, i + depth) for i, mod in enumerate(model.up_levels[li])]
    return steps


DROPOUT_SITE = 1 << 62          # the bit every dropout site id carries (include/kdiff_hip.h, mask contract)


def dropout_sites(model):
    """The model's dropout sites with a rate > 0, in forward order: (site id, step or mapping block, kind, p).  kind "attn": the attention
    output after the head merge, before out_proj (image_transformer_v2.py:394, :441, :474), site 2^62 | 2 i; "ff": the FF hidden after
    GEGLU, before down_proj (:491), site 2^62 | (2 i + 1) -- i the position of the layer's ``Step`` in ``hourglass(model)``, p its level's
    rate; "mapping": mapping block k's GEGLU output before down_proj (:564), site 2^62 | 2^32 | k, p the mapping dropout rate."""
    out = []
    for i, st in enumerate(hourglass(model)):
        p = model.level_specs[st.level].dropout if st.kind == "layer" else 0.0
        if p > 0:
            if hasattr(st.module, "self_attn"):
                out.append((DROPOUT_SITE | 2 * i, st, "attn", p))
            out.append((DROPOUT_SITE | (2 * i + 1), st, "ff", p))
    p = model.mapping_spec.dropout
    if p > 0:
        out += [(DROPOUT_SITE | 1 << 32 | k, k, "mapping", p) for k in range(len(model.mapping.blocks))]
    return out


def dropout_table(model, key):
    """{(layer prefix, "attn" | "ff") or ("mapping", block): (key, site, p)} of one loss call's dropout (``ops.dropout``'s arguments), for
    the primal and backward walks; {} without a key."""
    if key is None:
        return {}
    return {(("mapping", where) if kind == "mapping" else (where.prefix, kind)): (key, site, p) for site, where, kind, p in dropout_sites(model)}


def _level_pos(grids, li):
    """[h, w, 2] axial positions (y, x) of level ``li``'s tokens: cell centres of the top grid, 2x2 means below (:726, :52-54)."""
    h0, w0 = grids[0]
    pos = axial_rope.make_axial_pos(h0, w0).view(h0, w0, 2)
    for _ in range(li):
        pos = axial_rope.downscale_pos(pos)
    return pos


# ---------------------------------------------------------------------------------- the unfused ops path (dual and backward passes)

EPS = 1e-6


def conditioning(model, sigma, aug_cond, class_cond, mapping_cond, keep=None, drop=None):
    """The mapping network's output [B, mapping width] (image_transformer_v2.py:729-740, :552-581) on ``ops`` calls.  ``keep``: a dict
    that receives what the reverse of the chain needs (models/vjp.py): the Fourier features, the class ids, the mapping_cond rows, the
    norms' inputs.  ``drop``: a ``dropout_table`` whose mapping sites mask the blocks' GEGLU outputs (the training loss)."""
    m = model
    B = sigma.shape[0]
    dev = sigma.device
    ff = ops.fourier_sigma(sigma, m.time_emb.weight.detach().contiguous())
    temb = ops.linear(ff, m.time_in_proj.weight)
    aug = torch.zeros(B, 9, device=dev, dtype=torch.float32) if aug_cond is None else aug_cond.to(device=dev, dtype=torch.float32).reshape(B, 9).contiguous()
    aug_ff = ops.fourier_features(aug, m.aug_emb.weight.detach().contiguous())
    aug_proj = ops.linear(aug_ff, m.aug_in_proj.weight)
    emb = ids = None
    if m.class_emb is not None:
        ids = class_cond.to(device=dev, dtype=torch.int64).reshape(B).contiguous()
        lo, hi = (int(ids.min()), int(ids.max()))
        if lo < 0 or hi >= m.class_emb.weight.shape[0]:
            raise IndexError(f"class_cond ids must lie in [0, {m.class_emb.weight.shape[0] - 1}] (got {lo}..{hi})")
        emb = m.class_emb.weight
    mterm = None
    if m.mapping_cond_in_proj is not None:
        mrows = mapping_cond.to(device=dev, dtype=torch.float32).reshape(B, -1).contiguous()
        mterm = ops.linear(mrows, m.mapping_cond_in_proj.weight)
    c = ops.cond_sum(temb, aug_proj, emb=emb, ids=ids, c=mterm)
    if keep is not None:
        keep.update(time_ff=ff, aug_ff=aug_ff, ids=ids, mapping_rows=mrows if mterm is not None else None, blocks=[])
    c_sum = c
    c = ops.rms_norm(c, m.mapping.in_norm.scale)
    for k, blk in enumerate(m.mapping.blocks):
        if keep is not None:
            keep["blocks"].append(c)
        h = ops.norm_linear(c, blk.norm.scale, blk.up_proj.weight, rows_per_sample=B, epi=nat.EPI_GEGLU)
        dr = drop.get(("mapping", k)) if drop else None
        if dr is not None:
            ops.dropout(h, *dr, out=h)
        c = ops.linear(h, blk.down_proj.weight, residual=c)
    if keep is not None:
        keep.update(c_sum=c_sum, c_last=c)
    return ops.rms_norm(c, m.mapping.out_norm.scale)


def ada_scale(cond, norm):
    """AdaRMSNorm scales (:155-166): Linear(cond) + 1 -> [B, d]."""
    return ops.linear(cond, norm.linear.weight, out_add=1.0)


# ---------------------------------------------------------------------------------- kernel routing


@dataclass(frozen=True)
class LayerRoute:
    """The kernels of one layer (``route_layer``).  qkv: "attn_block" (projection + attention core in one launch), "proj_block",
    "mx8", "split" (kd_norm_split_f32 planes, then the GEMM), "plain" or None (no attention); core: the attention core's entry point
    (None: none, or inside the attention block); fuse_out: the out projection runs inside the FF kernel; ff: "kd_ffn_f32" /
    "kd_ffn_bf16" (one kernel) or "pair", whose up projection is routed like qkv (``up``) and whose down projection may be fp8;
    fuse_core: ``core`` and ``ff`` (with its fused out projection) run as ONE launch, kd_attn_ffn_f32."""
    qkv: Optional[str]
    core: Optional[str]
    fuse_out: bool
    ff: str
    up: Optional[str] = None
    down_mx8: bool = False
    fuse_core: bool = False


def _prepass(mode, width):
    """split3: widths the fused norm -> projection kernel (gemm_x3.hip) does not take (tiles of 128 features): their normalised rows
    travel as bf16 planes of their own (kd_norm_split_f32)."""
    return mode == nat.PREC_SPLIT3 and width not in (128, 256, 512) and width > 256 and width % 128 == 0 and width <= 2048


def _mx8_ok(lib, mode, M, N, K, epi):
    """fp8 mode: this norm -> projection goes to the block-scaled fp8 matrix instruction (kd_gemm_mx8)."""
    # (from 4 096 rows on -- library option mx8_min_rows: below that the few-rows bf16 kernels are ahead -- batch 1: 0.512 against 0.552 ms
    # per forward, profiles/r06_bench_detail_full.json)
    return mode == nat.PREC_FP8 and M >= lib.kd_get_option(b"mx8_min_rows", nat.OPTION_DEFAULT) and bool(lib.kd_gemm_mx8_supported(M, N, K, epi, 1))


def route_layer(lib, mode, B, T, rps, d, d_ff, nh, attn, switches, grid=None, kernel_size=None):
    """The kernels of a layer of width ``d`` over ``T`` = B x ``rps`` tokens in arithmetic mode ``mode`` (nat.PREC_*, PREC_FP8 included):
    ``attn`` is "global" / "neighborhood" / "shifted-window", or None for a layer without attention (``nh`` heads); ``switches`` maps
    the names of PLAN_SWITCHES to the plan's values; ``grid``: the level's token grid and ``kernel_size``: the neighbourhood's, where the
    caller knows them (without them no layer takes a form that depends on them).  Asks only host-side predicates of the library (``lib``):
    no tensors, no device."""
    bf = mode in (nat.PREC_BF16, nat.PREC_FP8)
    proj_block = bf and switches["KDIFF_PROJ_BLOCK"] != "0"
    ffn_x3 = mode == nat.PREC_SPLIT3 and bool(lib.kd_ffn_f32_supported(T, d, d_ff))      # (library option ffn_x3)
    ffn_bf = bf and bool(lib.kd_ffn_bf16_supported(T, d, d_ff))
    # out projection fused into the FF kernel: width 128 (+3.5 % images/s in round 3) and, since round 5, width 256 too: in round 3
    # that measured level (176.1 vs 176.0: one wave per SIMD there); with the round-4 / 5 kernels around it the removed launch + the
    # attention rows' HBM round trip are worth +1.5 .. +3.0 % on two boxes (same box, back to back: 207.9 / 207.9 / 208.7 vs 214.3;
    # 186.9 / 186.9 / 187.0 vs 189.4 / 190.0).  KDIFF_FFN_OUT: 0 never, 1 = width 128 only, all (default) = every width the kernel
    # takes, or ONE width
    fo = switches["KDIFF_FFN_OUT"]
    fuse_out = attn is not None and ((ffn_x3 and d in (128, 256)) or (ffn_bf and d == 128)) and (d == 128 if fo == "1" else fo in ("all", str(d)))
    qkv = core = None
    if attn is not None:
        # bf16 mode, global attention at 256 tokens per sample: norm -> qkv projection of a head -> cosine-sim + RoPE -> attention in
        # ONE launch per layer (csrc/block_bf16.hip: attn_block_bf16_kernel; q, k, v never reach HBM).  The descriptor is the qkv
        # projection's, its C the attention output
        # From 32 (sample, head) workgroups on: below that (batch 1 - 2 at level 2) the few-rows projection + the dense core are faster
        # (0.514 against 0.543 ms per forward at batch 1; from batch 4 on the one-launch form wins: profiles/r05_attn_block.md)
        # fp8 mode: the qkv projection on the fp8 matrix instruction -- except where the one-launch bf16 attention block takes the layer
        # (level 2 of the 256 x 256 configs: 25.5 us against 25.6 + 13.6 us for fp8 projection + dense core, profiles/r06_fp8_mode.md)
        if bf and attn == "global" and T % 256 == 0 and switches["KDIFF_ATTN_BLOCK"] != "0" and lib.kd_attn_block_bf16_supported(rps, d, nh) \
                and (B * nh >= 32 or switches["KDIFF_ATTN_BLOCK"] == "force"):
            qkv = "attn_block"
        elif _prepass(mode, d) and nh <= 16:
            # AdaRMSNorm -> planes once, then a GEMM whose two operands both move by LDS-DMA
            # (the tiled qkv epilogue keeps its per-head constants in a 16-head LDS table, csrc/gemm_x3t.hip: wider levels -- 1152 =
            # 18 heads and up -- take the fp32-A norm -> projection kernels of round 1 like every shape the fused kernels refuse)
            qkv = "split"
        elif _mx8_ok(lib, mode, T, 3 * d, d, nat.EPI_QKV):
            qkv = "mx8"
        elif proj_block and lib.kd_proj_block_bf16_supported(rps, d, 3 * d, nat.EPI_QKV) and 192 <= (T // 256) * (3 * d // 384) <= 256:
            # bf16 mode, K = 256 / 512 with an attention core of its own (neighbourhood / window levels): the projection in the block
            # form (kd_proj_block_bf16: a workgroup per (256-row group, 6 head vectors), rows normalised once) for one-round grids (192 .. 256)
            qkv = "proj_block"
        else:
            qkv = "plain"
        if qkv != "attn_block":
            core = f"kd_{_CORE[attn]}_{'bf16' if bf else 'f32'}"
    if ffn_x3 or ffn_bf:
        # the whole FeedForwardBlock (:487-493) in one kernel (csrc/ffn_x3.hip, csrc/ffn_bf16.hip): the d_ff-wide hidden activation stays
        # on the chip
        # split3, neighbourhood core followed by the width-128 FF kernel with its fused out projection (level 0 of the 256 x 256 configs):
        # both in ONE launch on the core's query tiles (csrc/attn_ffn_x3.hip: the attention rows never cross HBM; same bits).
        # KDIFF_ATTN_FFN=0: the two launches
        fuse_core = bool(ffn_x3 and fuse_out and attn == "neighborhood" and core == "kd_attn_na2d_f32" and grid is not None
                         and kernel_size is not None and switches.get("KDIFF_ATTN_FFN", "1") != "0"
                         and lib.kd_attn_ffn_f32_supported(B, grid[0], grid[1], nh, kernel_size, d, d_ff))
        return LayerRoute(qkv, core, fuse_out, "kd_ffn_f32" if ffn_x3 else "kd_ffn_bf16", fuse_core=fuse_core)
    if _prepass(mode, d) and d_ff % 64 == 0:
        return LayerRoute(qkv, core, fuse_out, "pair", "split")
    # fp8 mode: the hidden activation leaves the GEGLU epilogue as e4m3 rows + one power-of-two scale per (row, 32 features) -- in
    # the first half of `hid`, the scale bytes behind them -- and the down projection takes both operands as e4m3 by LDS-DMA
    up_mx8 = _mx8_ok(lib, mode, T, d_ff, d, nat.EPI_GEGLU)
    down_mx8 = up_mx8 and d_ff % 128 == 0 and bool(lib.kd_gemm_mx8_supported(T, d, d_ff, nat.EPI_RESIDUAL, 0))
    if up_mx8:
        up = "mx8"
    elif proj_block and lib.kd_proj_block_bf16_supported(rps, d, d_ff, nat.EPI_GEGLU) and 192 <= (T // 256) * (d_ff // 192) <= 256:
        # bf16 mode, rows per sample a multiple of 256: the projection in the attention block's form (a workgroup per (256-row group,
        # 192-output slice), rows normalised once; csrc/block_bf16.hip: proj_block_bf16_kernel) for grids that fill ONE round of the
        # chip's 256 CUs (192 .. 256 workgroups): two rounds measured level with the A-stationary kernel (42.3 against 41.5 us at
        # level 1), and a workgroup's six passes are a serial chain -- at 32 - 128 workgroups the A-stationary kernel, which splits
        # the same work over up to 512 slots, is faster (batch 4: 0.645 against 0.759 ms per forward; batch 16: level); same bits
        up = "proj_block"
    else:
        up = "plain"
    return LayerRoute(qkv, core, fuse_out, "pair", up, down_mx8)


# ---------------------------------------------------------------------------------- the plan

class _Launch:
    """One launch: entry point, its arguments without the stream (nat.encode_call's form), a name for error messages."""
    __slots__ = ("name", "args", "what")

    def __init__(self, name, args, what):
        self.name, self.args, self.what = name, args, what

    def __call__(self, lib, stream):
        """Issue it directly: descriptors by reference, a patched pointer (_ScaleRef) as it is now."""
        return getattr(lib, self.name)(*[C.byref(a) if isinstance(a, C.Structure) else a.scale if isinstance(a, _ScaleRef) else a
                                         for a in self.args], stream)


class _ScaleRef:
    """A scale-table address passed as a plain argument (kd_norm_split_f32), patched per run like ``_Plan.norm_descs``' descriptors."""

    def __init__(self):
        self._scale, self._call, self._index = None, None, 0

    def bind_call(self, call, index):               # (nat.encode_call: this pointer lives in a kd_run_list entry too)
        self._call, self._index = call, index

    @property
    def scale(self):
        return self._scale

    @scale.setter
    def scale(self, v):
        self._scale = v
        if self._call is not None:
            self._call.p[self._index] = v


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class _CondChain:
    """Launch list + buffers of the conditioning chain for a fixed number of rows (one row per sample and model call).
    Every kernel of the chain works row by row (the products go through the per-row fp32 FMA kernel, KdGemm.per_row), so
    a row's scales do not depend on how many rows share the launches: B rows per solver step or steps x B rows at once."""

    def __init__(self, rows, lib):
        self.rows, self.lib, self.launches, self.keep = rows, lib, [], []
        self.c_sigma = self.class_ids = self.aug_in = self.map_in = self.d_scales = None

    def fill(self, sigma, aug_cond, class_cond, mapping_cond, repeat=1):
        """Inputs of the chain on the current stream.  ``sigma``: [rows] (or one value); the other tensors are per sample
        ([rows / repeat, ...]) and repeated for every step of a schedule."""
        rows = self.rows
        self.c_sigma.copy_(sigma.reshape(-1).expand(rows) if sigma.numel() == 1 else sigma.reshape(rows), non_blocking=True)
        B = rows // repeat
        if self.class_ids is not None and class_cond is not None:
            self.class_ids.view(repeat, B).copy_(class_cond.reshape(1, B).expand(repeat, B), non_blocking=True)
        if self.aug_in is not None:
            self.aug_in.view(repeat, B, 9).copy_(aug_cond.reshape(1, B, 9).expand(repeat, B, 9), non_blocking=True)
        if self.map_in is not None:
            self.map_in.view(repeat, B, -1).copy_(mapping_cond.reshape(1, B, -1).expand(repeat, B, -1), non_blocking=True)

    def run(self, table_ptr, stream):
        """Scales of every AdaRMSNorm of the network for every row -> [rows, scale_width] fp32 at ``table_ptr``."""
        self.d_scales.C = table_ptr
        for ln in self.launches:
            rc = ln(self.lib, stream)
            if rc:
                nat.check(rc, ln.what)


class _Plan:
    """Workspace + prebuilt launch list for one (batch, H, W, conditioning-kinds) combination."""

    def release(self):
        """Give the workspaces back NOW: a plan's launch lists and conditioning chains close over the plan and over each other (reference
        cycles), so dropping the last outside reference would leave ~20 MB per image allocated until Python's cycle collector happens to run.
        The caller (``weights.PlanCache``: eviction, ``_drop_plans``, rare events) runs the collector once behind this for the helper objects' own cycles."""
        self.__dict__.clear()

    def __init__(self, model, B, H, W, grids, has_aug, has_class, has_mapping_cond, device, mode, switches):
        """``grids``: the levels' token grids (``_token_grids``); ``mode``: the arithmetic mode (nat.PREC_*); ``switches``: the values of
        PLAN_SWITCHES by name (both from the plan key)."""
        self.lib = nat.lib()
        m = self.model = model
        self.mode, self.switches = mode, switches
        # fp8 mode: the bf16 plan with the norm -> qkv / norm -> GEGLU projections of the K = 256 / 512 levels on the fp8 matrix instruction
        self.precision = precision = nat.PREC_BF16 if mode == nat.PREC_FP8 else mode
        bf = precision == nat.PREC_BF16
        self.cond_precision = nat.PREC_SPLIT3 if bf else precision      # the per-sample conditioning chain stays fp32 in every mode
        self.has_aug, self.has_class, self.has_mapping_cond, self.device = has_aug, has_class, has_mapping_cond, device
        self.keep = []           # tensors that must outlive the plan (descriptors live in the launches)
        self.launches = []
        f32 = dict(device=device, dtype=torch.float32)
        act = dict(device=device, dtype=torch.bfloat16 if bf else torch.float32)   # residual stream, qkv, attention out, FF hidden
        ph, pw = m.patch_size
        levels = self.levels = m.level_specs
        self.B, self.grids = B, grids
        self.out_shape = (B, m.out_channels, H, W)
        self.class_checked = {}                             # identities of the range-checked class_cond tensors (_plan_for) -> the tensor

        # ---- static buffers -----------------------------------------------------------------
        self.sigma = torch.empty(B, **f32)                  # preconditioning sigmas of the MAIN chain when the caller's cannot be read in place
        self.sigma_ptr = self.sigma.data_ptr()
        self.xs = xs = [torch.empty(B, gh, gw, lv.width, **act) for (gh, gw), lv in zip(grids, levels)]
        self.toks = toks = [B * gh * gw for gh, gw in grids]
        self.qkv = torch.empty(max(t * 3 * lv.width for t, lv in zip(toks, levels)), **act)
        self.att = torch.empty(max(t * lv.width for t, lv in zip(toks, levels)), **act)
        self.hid = torch.empty(max(t * lv.d_ff for t, lv in zip(toks, levels)), **act)
        # fp32-parity mode, round 3: GEMM operands that a producer can split once travel as two bf16 planes (hi, lo: the same bytes as
        # fp32) and the consumer GEMM moves them by LDS-DMA (csrc/gemm_x3t.hip).  Planes of the FF hidden activation live in `hid`
        # (hi in its first half, lo in the second); the normalised rows of the levels whose width exceeds the fused norm -> projection
        # kernel's register budget (> 256) get planes of their own (`xn`, written by kd_norm_split_f32).
        wide = [t * lv.width for t, lv in zip(toks, levels) if _prepass(mode, lv.width)]
        self.xn = torch.empty(max(wide), **f32) if wide else None
        norm_mods = m._ada_norm_modules()
        self.table_offsets, total = {}, 0                  # byte offset of each AdaRMSNorm's scales in a scale table row
        for name, mod in norm_mods:
            self.table_offsets[name] = 4 * total
            total += mod.linear.weight.shape[0]
        # one concatenation of the AdaRMSNorm projections per MODEL, not per plan: it is a function of the weights only, and the packed-image
        # cache keeps its source alive -- made per plan, every batch size ever seen left 2 x 7.5 MB behind (256 x 256 configs) until the
        # weights changed.  (model._packed goes with the plans whenever the weights do.)
        wcat = m._packed.get("ada_norm_wcat")
        if wcat is None or wcat.device != device:
            wcat = m._packed["ada_norm_wcat"] = torch.cat([mod.linear.weight.detach() for _, mod in norm_mods], dim=0).contiguous()
        self.wcat = wcat
        self.norm_descs = []                                # (descriptor or _ScaleRef, byte offset into a scale table)
        self.scale_width = total                            # of a scale table row (laid out by ``table_offsets``)
        self.tables = ScaleTables(B, total, device, self.build_cond)      # which table a call reads, and what fills it on which stream

        # ---- hourglass ------------------------------------------------------------------------
        L = self.launches
        self.d_patch_in = self._gemm(L, "patch_in", None, m.patch_in.proj.weight, xs[0], toks[0], levels[0].width, m.in_channels * ph * pw,
                                     a_mode=nat.A_PATCH_NCHW, grid=grids[0], patch=(ph, pw, m.in_channels))
        for st in hourglass(m):
            li = st.level
            if st.kind == "layer":
                self._add_layer(li, st.prefix, st.module, st.index)
            elif st.kind == "merge":
                self._gemm(L, f"merges.{li}", xs[li], m.merges[li].proj.weight, xs[li + 1], toks[li + 1], levels[li + 1].width,
                           4 * levels[li].width, a_mode=nat.A_MERGE2x2, grid=grids[li + 1])
            else:
                self._gemm(L, f"splits.{li}", xs[li + 1], m.splits[li].proj.weight, xs[li], toks[li + 1], 4 * levels[li].width,
                           levels[li + 1].width, epi=nat.EPI_SPLIT_LERP, residual=xs[li], fac=m.splits[li].fac, grid=grids[li + 1])
        self.d_patch_out = self._gemm(L, "patch_out", xs[0], m.patch_out.proj.weight, None, toks[0], m.out_channels * ph * pw,
                                      levels[0].width, epi=nat.EPI_UNPATCH_NCHW, norm_scale=m.out_norm.scale, scale_stride=0,
                                      rows_per_sample=grids[0][0] * grids[0][1], grid=grids[0], patch=(ph, pw, m.out_channels))
        self._encode_launches()

    def _gemm(self, launches, what, A, Wt, Cc, M, N, K, cond=False, table=None, entry=None, mx8=False, **kw):
        """An ``ops.gemm`` descriptor (weight images from the model's cache) appended to ``launches`` as a launch of ``entry`` (default: the
        plain GEMM of its precision).  ``cond``: a product of a conditioning chain (fp32 in every mode, one row per sample: _CondChain);
        ``table``: name of the AdaRMSNorm whose scales it reads from the live scale table (the address is patched per run)."""
        precision = self.cond_precision if cond else self.precision
        if table is not None:
            kw.update(scale_ptr=0, scale_stride=self.scale_width)
        d = ops.gemm(A, Wt, Cc, M=M, N=N, K=K, precision=precision, per_row=cond, mx8=mx8, launch=False, pack=self.model._packed_image, **kw)
        if table is not None:
            self.norm_descs.append((d, self.table_offsets[table]))
        launches.append(_Launch(entry or ops._gemm_entry(precision, mx8), (d,), what + ("(mx8)" if mx8 else "")))
        return d

    def _norm_split(self, launches, table, x, T, d, rps):
        """AdaRMSNorm ``table`` of the fp32 rows of ``x`` -> (hi, lo) bf16 planes in ``xn`` (kd_norm_split_f32)."""
        ref = _ScaleRef()
        self.norm_descs.append((ref, self.table_offsets[table]))
        planes = self.xn.view(torch.bfloat16)
        hi, lo = planes[:T * d], planes[T * d:2 * T * d]
        launches.append(_Launch("kd_norm_split_f32", (_ptr(x), ref, self.scale_width, rps, _ptr(hi), _ptr(lo), T, d, 1e-6), table + " (split)"))
        return hi, lo

    def build_cond(self, rows):
        """The conditioning chain (image_transformer_v2.py:734-740, :569-581) for ``rows`` rows: FourierFeatures ->
        mapping network -> every AdaRMSNorm scale of the network, with its own input and work buffers."""
        m, f32 = self.model, dict(device=self.device, dtype=torch.float32)
        mw, mdff = m.mapping_spec.width, m.mapping_spec.d_ff
        ch = _CondChain(rows, self.lib)
        L = ch.launches
        ch.c_sigma = torch.empty(rows, **f32)
        ch.class_ids = torch.zeros(rows, device=self.device, dtype=torch.int64)
        ch.aug_in = torch.zeros(rows, 9, **f32) if self.has_aug else None
        ch.map_in = torch.zeros(rows, m.mapping_cond_dim, **f32) if self.has_mapping_cond else None
        ff, temb, emb, mres, cond = (torch.empty(rows, mw, **f32) for _ in range(5))
        mh = torch.empty(rows, mdff, **f32)
        ch.keep += [ff, temb, emb, mres, cond, mh]
        L.append(_Launch("kd_fourier_sigma_f32", (_ptr(ch.c_sigma), _ptr(m.time_emb.weight), _ptr(ff), rows, mw // 2), "fourier_sigma"))
        self._gemm(L, "time_in_proj", ff, m.time_in_proj.weight, temb, rows, mw, mw, cond=True)
        if self.has_aug:
            aug_ff, aug_proj = torch.empty(rows, mw, **f32), torch.empty(rows, mw, **f32)
            ch.keep += [aug_ff, aug_proj]
            L.append(_Launch("kd_fourier_f32", (_ptr(ch.aug_in), _ptr(m.aug_emb.weight), _ptr(aug_ff), rows, 9, mw // 2), "fourier_aug"))
            self._gemm(L, "aug_in_proj", aug_ff, m.aug_in_proj.weight, aug_proj, rows, mw, mw, cond=True)
            aug_term, aug_rows = aug_proj, 1
        else:
            # aug_cond = zeros  =>  FourierFeatures = [cos 0, sin 0] = [1..1, 0..0]: a constant vector
            z_ff, aug_const = torch.empty(1, mw, **f32), torch.empty(1, mw, **f32)
            zeros9 = torch.zeros(1, 9, **f32)
            ch.keep += [z_ff, aug_const, zeros9]
            L.append(_Launch("kd_fourier_f32", (_ptr(zeros9), _ptr(m.aug_emb.weight), _ptr(z_ff), 1, 9, mw // 2), "fourier_aug0"))
            self._gemm(L, "aug_in_proj0", z_ff, m.aug_in_proj.weight, aug_const, 1, mw, mw, cond=True)
            aug_term, aug_rows = aug_const, 0
        map_term = None
        if self.has_mapping_cond:
            map_term = torch.empty(rows, mw, **f32)
            ch.keep.append(map_term)
            self._gemm(L, "mapping_cond_in_proj", ch.map_in, m.mapping_cond_in_proj.weight, map_term, rows, mw, m.mapping_cond_dim, cond=True)
        L.append(_Launch("kd_cond_sum_f32", (_ptr(emb), _ptr(temb), _ptr(aug_term), aug_rows,
                                             _ptr(m.class_emb.weight) if self.has_class else None, _ptr(ch.class_ids) if self.has_class else None,
                                             None if map_term is None else _ptr(map_term), rows, mw), "cond_sum"))
        L.append(_Launch("kd_rmsnorm_f32", (_ptr(emb), _ptr(m.mapping.in_norm.scale), _ptr(mres), rows, mw, C.c_float(1e-6)), "mapping.in_norm"))
        for blk in m.mapping.blocks:
            self._gemm(L, "mapping.up_proj", mres, blk.up_proj.weight, mh, rows, mdff, mw, cond=True, epi=nat.EPI_GEGLU,
                       norm_scale=blk.norm.scale, scale_stride=0, rows_per_sample=rows)
            self._gemm(L, "mapping.down_proj", mh, blk.down_proj.weight, mres, rows, mw, mdff, cond=True, epi=nat.EPI_RESIDUAL, residual=mres)
        L.append(_Launch("kd_rmsnorm_f32", (_ptr(mres), _ptr(m.mapping.out_norm.scale), _ptr(cond), rows, mw, C.c_float(1e-6)), "mapping.out_norm"))
        ch.d_scales = self._gemm(L, "ada_norm_scales", cond, self.wcat, None, rows, self.scale_width, mw, cond=True, out_add=1.0)
        return ch

    def _qk(self, li, sa, nh):
        """Per-head constants of the qkv epilogue: (cosine-sim scale, RoPE tables, nh[, positions, frequencies])."""
        m = self.model
        if self.precision == nat.PREC_BF16:
            # bf16 mode: the qkv epilogue evaluates the RoPE angles itself (hardware sin / cos) from the token's axial
            # position and the head's frequencies in revolutions -- two tiny tables instead of cos / sin per (token, head)
            cos_t, sin_t = m._rope(li, self.grids, sa, self.device, revs=True)
        else:
            cos_t, sin_t = m._rope(li, self.grids, sa, self.device)
        self.keep += [cos_t, sin_t]
        qk = (sa.scale, cos_t, sin_t, nh)
        if self.precision == nat.PREC_SPLIT3:
            # the split3 projections of round 3 evaluate the angles like the bf16 ones (no table loads beside their LDS-DMA ring);
            # the tables stay for the round-1 kernels they fall back to (ragged shapes) and for the exact mode
            pos_t, freq_t = m._rope(li, self.grids, sa, self.device, revs=True)
            self.keep += [pos_t, freq_t]
            qk += (pos_t, freq_t)
        return qk

    def _add_layer(self, li, prefix, mod, index):
        L, lv, (gh, gw), T = self.launches, self.levels[li], self.grids[li], self.toks[li]
        d, d_ff, x, rps = lv.width, lv.d_ff, self.xs[li], gh * gw
        spec = lv.self_attn
        nh = d // spec.d_head if hasattr(mod, "self_attn") else 0
        kind, core, params = attn_geometry(spec, index) if nh else (None, None, ())
        r = route_layer(self.lib, self.mode, self.B, T, rps, d, d_ff, nh, kind, self.switches, grid=(gh, gw),
                        kernel_size=params[0] if kind == "neighborhood" else None)
        split3 = self.precision == nat.PREC_SPLIT3
        if nh:
            sa, norm = mod.self_attn, prefix + "self_attn.norm"
            # q, k leave the qkv GEMM already prepared (cosine-sim scale + RoPE in its epilogue): every halo /
            # window / key tile of the attention cores would otherwise redo that work per use
            # ... and, for the split-bf16x3 cores, already SPLIT (hi / lo bf16 chunks in the fp32 slots): the cores take
            # their operands as stored instead of converting every halo / window / key-block element again
            q = dict(epi=nat.EPI_QKV, rows_per_sample=rps, qk=self._qk(li, sa, nh), qkv_packed=split3)
            if r.qkv == "attn_block":
                self._gemm(L, prefix + "attn_block", x, sa.qkv_proj.weight, self.att, T, 3 * d, d, table=norm, entry="kd_attn_block_bf16", **q)
            elif r.qkv == "split":
                planes = self._norm_split(L, norm, x, T, d, rps)
                self._gemm(L, prefix + "qkv_proj", None, sa.qkv_proj.weight, self.qkv, T, 3 * d, d, a_planes=planes, **q)
            elif r.qkv == "proj_block":
                self._gemm(L, prefix + "qkv_proj(block)", x, sa.qkv_proj.weight, self.qkv, T, 3 * d, d, table=norm, entry="kd_proj_block_bf16", **q)
            else:
                self._gemm(L, prefix + "qkv_proj", x, sa.qkv_proj.weight, self.qkv, T, 3 * d, d, table=norm, mx8=r.qkv == "mx8", **q)
            if r.core is not None and not r.fuse_core:
                geo = ((rps, nh) if kind == "global" else (gh, gw, nh)) + params
                prep = () if r.core.endswith("_bf16") else (2 if split3 else 0, None, None, None, C.c_float(1e-6), self.precision)
                L.append(_Launch(r.core, (_ptr(self.qkv), _ptr(self.att), self.B, *geo, *prep), prefix + core))
            if not r.fuse_out:
                self._gemm(L, prefix + "out_proj", self.att, sa.out_proj.weight, x, T, d, d, epi=nat.EPI_RESIDUAL, residual=x)
        norm, w_up, w_down = prefix + "ff.norm", mod.ff.up_proj.weight, mod.ff.down_proj.weight
        if r.ff != "pair":
            # the whole FeedForwardBlock in one kernel; with r.fuse_out the attention block's out projection runs in front of it in the same
            # kernel (x + att W_out^T never crosses HBM)
            fd = ops.ffn(x, None, w_up, w_down, out=x, scale_stride=self.scale_width, rows_per_sample=rps, attn=self.att if r.fuse_out else None,
                         w_out=mod.self_attn.out_proj.weight if r.fuse_out else None, launch=False, pack=self.model._packed_image)
            self.norm_descs.append((fd, self.table_offsets[norm]))
            if r.fuse_core:
                L.append(_Launch("kd_attn_ffn_f32", (_ptr(self.qkv), fd, self.B, gh, gw, nh, *params), prefix + core + "+ff"))
            else:
                L.append(_Launch(r.ff, (fd,), prefix + "ff"))
            return
        hid8 = None
        if r.up == "split":
            planes = self._norm_split(L, norm, x, T, d, rps)
            self._gemm(L, prefix + "up_proj", None, w_up, self.hid, T, d_ff, d, epi=nat.EPI_GEGLU, a_planes=planes)
        else:
            if r.down_mx8:                                  # (e4m3 rows, scale bytes behind them) in `hid`
                b = self.hid.view(torch.uint8)
                hid8 = (b[:T * d_ff], b[T * d_ff:T * d_ff + T * d_ff // 32])
            block = r.up == "proj_block"
            self._gemm(L, prefix + ("up_proj(block)" if block else "up_proj"), x, w_up, self.hid, T, d_ff, d, epi=nat.EPI_GEGLU, table=norm,
                       rows_per_sample=rps, mx8=r.up == "mx8", c_planes=hid8, entry="kd_proj_block_bf16" if block else None)
        if r.down_mx8:
            self._gemm(L, prefix + "down_proj", None, w_down, x, T, d, d_ff, epi=nat.EPI_RESIDUAL, residual=x, a_planes=hid8, mx8=True)
        else:
            self._gemm(L, prefix + "down_proj", self.hid, w_down, x, T, d, d_ff, epi=nat.EPI_RESIDUAL, residual=x)

    def run(self, x, out, sigma_data, base):
        """Main chain on the current stream.  x: input image (read by patch_in and, when preconditioning, by patch_out);
        out: result image; ``self.sigma_ptr`` was set by the caller; the [B, scale_width] table at ``base`` holds this
        step's AdaRMSNorm scales."""
        for d, off in self.norm_descs:
            d.scale = base + off
        pin, pout = self.d_patch_in, self.d_patch_out
        pin.A = x.data_ptr()
        pout.C = out.data_ptr()
        if sigma_data is None:
            pin.sigma, pout.sigma, pout.R = None, None, None
        else:
            sp = self.sigma_ptr
            pin.sigma, pout.sigma, pout.R = sp, sp, x.data_ptr()
            pin.sigma_data = pout.sigma_data = float(sigma_data)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.calls is not None:
            # the whole list in one host call (kd_run_list): ~6.5 us of Python / ctypes per launch otherwise, which at batch 1 - 2 is more
            # than the kernels of the bf16 mode take
            rc = self.run_list(self.calls, len(self.launches), stream, C.byref(self.failed))
            if rc:
                nat.check(rc, self.launches[self.failed.value].what)
            return
        for ln in self.launches:
            rc = ln(self.lib, stream)
            if rc:
                nat.check(rc, ln.what)

    def _encode_launches(self):
        """The main chain as a kd_run_list array, if every launch of it can be named there (and KDIFF_RUN_LIST is not 0)."""
        self.calls, self.failed, self.run_list = None, C.c_int(0), self.lib.kd_run_list
        if self.switches["KDIFF_RUN_LIST"] == "0" or not self.launches:
            return
        calls = (nat.KdCall * len(self.launches))()
        for call, ln in zip(calls, self.launches):
            if not nat.encode_call(call, ln.name, ln.args):
                return
        self.calls = calls


# ---------------------------------------------------------------------------------- the model

def _wants_input_grad(x):
    return torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad


class _InputGrad(torch.autograd.Function):
    """The model as an autograd node with x its only differentiable input.  Forward: ``_run`` with its launch plan (the same bits as a
    no-grad call); saved: the inputs only (x, sigma, the conditioning), no activations.  Backward: ``vjp.backward`` recomputes the primal
    and returns J^T grad for x."""

    @staticmethod
    def forward(ctx, x, model, sigma, aug_cond, class_cond, mapping_cond, sigma_data):
        for name, t in (("sigma", sigma), ("aug_cond", aug_cond), ("class_cond", class_cond), ("mapping_cond", mapping_cond)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f"ImageTransformerDenoiserModelV2: gradients w.r.t. {name} are not implemented (the backward pass "
                                          f"differentiates w.r.t. the input x only); pass {name}.detach()")
        out = model._run(x, sigma, aug_cond, class_cond, mapping_cond, sigma_data)
        ctx.model, ctx.sigma_data = model, sigma_data
        ctx.save_for_backward(x, sigma, aug_cond, class_cond, mapping_cond)
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import vjp
        x, sigma, aug_cond, class_cond, mapping_cond = ctx.saved_tensors
        gx = vjp.backward(ctx.model, x, sigma, grad.to(torch.float32).contiguous(), aug_cond=aug_cond, class_cond=class_cond,
                          mapping_cond=mapping_cond, sigma_data=ctx.sigma_data)
        return gx, None, None, None, None, None, None


class _ParamGrad(torch.autograd.Function):
    """The inner model as an autograd node whose differentiable inputs are its parameters (``Denoiser.loss`` only).  Forward: the fp32
    ``ops``-path primal (``vjp.primal``); saved: the inputs, no activations.  Backward: ``vjp.backward`` with the parameters autograd asks
    for; the rest cost nothing."""

    @staticmethod
    def forward(ctx, x, model, sigma, aug_cond, class_cond, mapping_cond, key, *params):
        from . import vjp
        out = vjp.primal(model, x, sigma, aug_cond, class_cond, mapping_cond, dropout=key)
        ctx.model, ctx.params = model, params
        ctx.save_for_backward(x, sigma, aug_cond, class_cond, mapping_cond, key)     # the key: the recomputation draws the same masks
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import vjp
        x, sigma, aug_cond, class_cond, mapping_cond, key = ctx.saved_tensors
        need = ctx.needs_input_grad[7:]
        want = [p for p, n in zip(ctx.params, need) if n]
        _, grads = vjp.backward(ctx.model, x, sigma, grad.to(torch.float32).contiguous(), aug_cond=aug_cond, class_cond=class_cond,
                                mapping_cond=mapping_cond, params=want, dropout=key)
        return (None,) * 7 + tuple(grads.get(id(p)) if n else None for p, n in zip(ctx.params, need))


class ImageTransformerDenoiserModelV2(nn.Module):
    def __init__(self, levels, mapping, in_channels, out_channels, patch_size, num_classes=0, mapping_cond_dim=0):
        super().__init__()
        for lv in levels:
            sa = lv.self_attn
            if not isinstance(sa, (GlobalAttentionSpec, NeighborhoodAttentionSpec, ShiftedWindowAttentionSpec, NoAttentionSpec)):
                raise ValueError(f"unsupported self attention spec {sa}")
            if not isinstance(sa, NoAttentionSpec) and sa.d_head != D_HEAD:
                raise ValueError(f"d_head must be {D_HEAD} (got {sa.d_head}): the HIP kernels of both arithmetic modes -- qkv epilogue (cosine-sim "
                                 f"norm + RoPE over {D_HEAD // 2} dims), attention cores, qkv layout [tokens, 3, n_heads, {D_HEAD}] of "
                                 f"include/kdiff_hip.h -- are built for {D_HEAD}-dim heads, as every shipped config uses (config.py:137-138); "
                                 f"the reference's other head sizes (image_transformer_v2.py:355-363) are not supported")
            if not isinstance(sa, NoAttentionSpec) and lv.width % sa.d_head:
                raise ValueError(f"width {lv.width} is not a multiple of d_head {sa.d_head}")
        self.level_specs, self.mapping_spec = list(levels), mapping
        self.in_channels, self.out_channels = in_channels, out_channels
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.num_classes, self.mapping_cond_dim = num_classes, mapping_cond_dim
        ph, pw = self.patch_size
        mw = mapping.width

        self.patch_in = _Holder(proj=_linear_weight(levels[0].width, in_channels * ph * pw))
        self.time_emb = _Holder(weight=torch.randn(mw // 2, 1))
        self.time_in_proj = _linear_weight(mw, mw)
        self.aug_emb = _Holder(weight=torch.randn(mw // 2, 9))
        self.aug_in_proj = _linear_weight(mw, mw)
        self.class_emb = _Holder(weight=nn.Parameter(torch.randn(num_classes, mw))) if num_classes else None
        self.mapping_cond_in_proj = _linear_weight(mw, mapping_cond_dim) if mapping_cond_dim else None
        self.mapping = _Holder(
            in_norm=_rms_scale(mw),
            blocks=nn.ModuleList([_Holder(norm=_rms_scale(mw), up_proj=_linear_weight(2 * mapping.d_ff, mw),
                                          down_proj=_linear_weight(mw, mapping.d_ff, zero=True)) for _ in range(mapping.depth)]),
            out_norm=_rms_scale(mw))
        self.down_levels, self.up_levels = nn.ModuleList(), nn.ModuleList()
        for i, lv in enumerate(levels):
            if i < len(levels) - 1:
                self.down_levels.append(nn.ModuleList([_layer(lv, mw) for _ in range(lv.depth)]))
                self.up_levels.append(nn.ModuleList([_layer(lv, mw) for _ in range(lv.depth)]))
            else:
                self.mid_level = nn.ModuleList([_layer(lv, mw) for _ in range(lv.depth)])
        self.merges = nn.ModuleList([_Holder(proj=_linear_weight(b.width, 4 * a.width)) for a, b in zip(levels[:-1], levels[1:])])
        self.splits = nn.ModuleList([_Holder(proj=_linear_weight(4 * a.width, b.width), fac=nn.Parameter(torch.ones(1) * 0.5))
                                     for a, b in zip(levels[:-1], levels[1:])])
        self.out_norm = _rms_scale(levels[0].width)
        self.patch_out = _Holder(proj=_linear_weight(out_channels * ph * pw, levels[0].width, zero=True))
        self._watch, self._plan_cache = weights.WeightWatch(self), weights.PlanCache()
        self._plans = self._plan_cache.plans                # the plain dict, by key, most recently used last
        self._fingerprint, self._packed, self._derived, self._plans_epoch = None, {}, {}, None
        self._dropout_on, self._dropout_gen = False, None
        self.wgrad_arithmetic = None

    # ---- bookkeeping ---------------------------------------------------------------------------
    def _ada_norm_modules(self):
        out = []

        def visit(prefix, layers):
            for i, mod in enumerate(layers):
                if hasattr(mod, "self_attn"):
                    out.append((f"{prefix}{i}.self_attn.norm", mod.self_attn.norm))
                out.append((f"{prefix}{i}.ff.norm", mod.ff.norm))
        for li, lvl in enumerate(self.down_levels):
            visit(f"down_levels.{li}.", lvl)
        for li, lvl in enumerate(self.up_levels):
            visit(f"up_levels.{li}.", lvl)
        visit("mid_level.", self.mid_level)
        return out

    def _derive(self, tag, sources, build):
        """``build()``: tensors derived from the weights ``sources`` alone, kept per model under ``tag`` and the sources' identities and
        version counters, so an in-place edit of a source builds them again (tensors made under torch.inference_mode() carry no counter:
        ``invalidate()``).  The entry keeps its sources alive, so their ids cannot be recycled under it.  The store goes with ``_packed``
        whenever the weights change, and at ``invalidate()``.  (A lookup does not read ``_weights_fingerprint``: 25 - 30 us per call.)"""
        key = (tag, *[weights.ident(t, never_same=False) for t in sources])
        ent = self._derived.get(key)
        if ent is None:
            if len(self._derived) >= DERIVED_KEPT:
                self._derived.clear()
            ent = self._derived[key] = (sources, build())
        return ent[1]

    def _rope(self, li, grids, sa, device, revs=False):
        """AxialRoPE operands of attention ``sa`` at level ``li`` of ``grids``, evaluated on the CPU in fp32 (axial_rope): (cos, sin)
        tables [tokens, nh, 16], or with ``revs`` ([tokens, 2] positions (y, x), [nh, 8] frequencies in revolutions) for the kernels that
        evaluate the angles themselves."""
        freqs = sa.pos_emb.freqs

        def build():
            pos = _level_pos(grids, li)
            if revs:
                freq = freqs.detach().to(torch.float32).cpu() / (2.0 * math.pi)
                return pos.reshape(-1, 2).to(torch.float32).contiguous().to(device), freq.contiguous().to(device)
            cos_t, sin_t = axial_rope.rope_tables(pos, freqs.detach())
            return cos_t.to(device), sin_t.to(device)
        return self._derive(("rope", li, grids[0], device, revs), (freqs,), build)

    def _drop_plans(self):
        """All cached plans go, workspaces at once (``_Plan.release``), each plan's device idle first."""
        self._plan_cache.drop_all()

    def invalidate(self):
        """Drop the plans and packed weight images at the next call.  Needed only after an IN-PLACE edit of weights that were created
        under torch.inference_mode() outside load_state_dict / .to(): such tensors carry no version counter, so the edit leaves no trace
        (_weights_fingerprint sees everything else by itself).  The tensors the dual and backward passes derive from the weights
        (``_derive``) go at once."""
        self._watch.bump()
        self._derived = {}

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .half(): the same Parameter objects with new .data (seen through their addresses) or, with
        # torch.__future__.set_overwrite_module_params_on_conversion(True), new Parameters in the dicts (seen through the slot check);
        # the epoch covers inference-mode tensors converted in place
        out = super()._apply(fn, *args, **kwargs)
        self._watch.bump()
        return out

    def _packed_image(self, W, N, K, geglu, bf16=False):
        """Packed image of a weight (split-bf16, or plain bf16 for the bf16 mode), shared by all plans of this model.  The
        entry keeps the source tensor alive, so its address cannot be recycled under the cached image; the dict is dropped
        with the plans whenever the weights change (``_weights_fingerprint``)."""
        key = (id(W), N, K, int(geglu), bf16 if bf16 == "mx8" else bool(bf16))
        ent = self._packed.get(key)
        if ent is None:
            ent = self._packed[key] = (W, ops.pack_weight(W, N, K, geglu, cache=False, bf16=bf16))
        return ent[1]

    def _weights_fingerprint(self):
        """``weights.WeightWatch.fingerprint`` of this model's tree: read on every model call."""
        return self._watch.fingerprint()

    def _param_tags(self, name):
        """The reference's parameter tags (image_transformer_v2.py:59-84): "wd" on the weights of the projections, "mapping" on the mapping
        network and the AdaRMSNorm projections (:159-160, :680)."""
        tags = set()
        if name.endswith(".weight") and not name.startswith(("time_in_proj.", "aug_in_proj.", "class_emb.", "mapping_cond_in_proj.")):
            tags.add("wd")
        if name.startswith("mapping.") or name.endswith(".norm.linear.weight"):
            tags.add("mapping")
        return tags

    def param_groups(self, base_lr=5e-4, mapping_lr_scale=1 / 3):
        """The reference's four AdamW groups (image_transformer_v2.py:708-719): weight-decayed and not, each at ``base_lr`` or, for the
        mapping network and the AdaRMSNorm projections, at ``base_lr * mapping_lr_scale``."""
        groups = {(wd, mp): [] for mp in (False, True) for wd in (True, False)}
        for name, p in self.named_parameters():
            tags = self._param_tags(name)
            groups[("wd" in tags, "mapping" in tags)].append(p)
        return [
            {"params": groups[(True, False)], "lr": base_lr},
            {"params": groups[(False, False)], "lr": base_lr, "weight_decay": 0.0},
            {"params": groups[(True, True)], "lr": base_lr * mapping_lr_scale},
            {"params": groups[(False, True)], "lr": base_lr * mapping_lr_scale, "weight_decay": 0.0},
        ]

    def _dropout_rates(self):
        return [(f"levels[{i}].dropout", lv.dropout) for i, lv in enumerate(self.level_specs)] + [("mapping dropout", self.mapping_spec.dropout)]

    def enable_dropout(self, generator=None):
        """Opt in to dropout in the training loss: from now on ``loss_forward`` (``Denoiser.loss``) of the model in training mode applies
        the config's dropout rates, on masks of this project's counter-based generator (include/kdiff_hip.h, mask contract) -- not torch's
        dropout RNG stream.  Each such call draws one int64 key from ``generator`` (a torch.Generator on the model's device; None: the
        default generator of the input's device, so torch.manual_seed governs it), as the reference's train.py draws its seeds; the
        backward pass regenerates the same masks from it.  While enabled, in training mode with a rate > 0, ``forward``,
        ``forward_preconditioned`` and ``forward_jvp`` raise (they have no dropout): call model.eval() for them.  The setting is not part of
        the state_dict.  Returns the model."""
        bad = [f"{name} = {p}" for name, p in self._dropout_rates() if not 0.0 <= p < 1.0]
        if bad:
            raise ValueError(f"ImageTransformerDenoiserModelV2.enable_dropout: dropout rates must lie in [0, 1) ({', '.join(bad)})")
        if generator is not None and not isinstance(generator, torch.Generator):
            raise TypeError(f"enable_dropout: generator must be a torch.Generator or None (got {type(generator)})")
        self._dropout_on, self._dropout_gen = True, generator
        return self

    def set_wgrad_arithmetic(self, arithmetic=None):
        """Opt in to bf16 weight gradients in the training loss.  ``None`` (the default): the backward pass's rule (split3, or exact fp32
        under KDIFF_GEMM=exact).  ``"bf16"``: every weight-gradient GEMM dW = G^T X of ``loss_forward``'s backward rounds both operands to
        bf16 after their prologue and accumulates in fp32, one MFMA per product (``ops.wgrad(bf16=True)``): a ``Linear`` backward of the
        reference under ``--mixed-precision bf16``.  Only those GEMMs move: the primal (so the loss), the data-gradient GEMMs, the
        attention rules, the column sums and the class embedding keep their fp32-grade arithmetic.  Honoured in every KDIFF_GEMM mode.
        The setting is not part of the state_dict.  Returns the model."""
        if arithmetic not in (None, "bf16"):
            raise ValueError(f"ImageTransformerDenoiserModelV2.set_wgrad_arithmetic: {arithmetic!r} (None or 'bf16')")
        self.wgrad_arithmetic = arithmetic
        return self

    def _dropout_applies(self):
        return self.training and any(p > 0 for _, p in self._dropout_rates())

    def _refuse_when_dropping(self, what):
        if self._dropout_on and self._dropout_applies():
            raise NotImplementedError(f"ImageTransformerDenoiserModelV2.{what}: dropout is enabled and the model is in training mode, and this "
                                      f"pass has no dropout; call model.eval() first (dropout applies to loss_forward / Denoiser.loss only)")

    def loss_forward(self, x, sigma, aug_cond=None, class_cond=None, mapping_cond=None):
        """F(x, sigma) for ``Denoiser.loss``: the fp32 ``ops``-path primal, in every arithmetic mode.  Under grad mode the output carries a
        ``grad_fn`` whose backward fills the ``.grad`` of every parameter that requires grad (models/vjp.py); x, sigma and the conditioning
        get none.  In training mode with a dropout rate > 0 the config's dropout applies once ``enable_dropout`` was called (one key drawn
        per call); without it the call raises."""
        key = None
        if self._dropout_applies():
            if not self._dropout_on:
                drop = [f"{name} = {p}" for name, p in self._dropout_rates() if p > 0]
                raise NotImplementedError(f"ImageTransformerDenoiserModelV2: dropout in training mode needs model.enable_dropout() "
                                          f"({', '.join(drop)}; masks from this project's counter-based generator); or call model.eval() "
                                          f"for the dropout-free objective")
            if isinstance(x, torch.Tensor) and x.is_cuda:        # (on the CPU the primal refuses the call below)
                key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=x.device, generator=self._dropout_gen)
        params = [p for p in self.parameters() if p.requires_grad] if torch.is_grad_enabled() else []
        if params:
            return _ParamGrad.apply(x, self, sigma, aug_cond, class_cond, mapping_cond, key, *params)
        from . import vjp
        return vjp.primal(self, x, sigma, aug_cond, class_cond, mapping_cond, dropout=key)

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, x, sigma, aug_cond=None, class_cond=None, mapping_cond=None):
        """Inner model F(x, sigma): [B, C, H, W] fp32 on a ROCm device -> [B, C, H, W].

        Under grad mode with ``x.requires_grad`` the output carries a ``grad_fn`` whose backward is J^T grad w.r.t. x (models/vjp.py);
        the output itself is the same bits as without grad.  Gradients go to x only: the parameters get none (their ``.grad`` stays None;
        parameter gradients go through ``Denoiser.loss``, see ``loss_forward``), and sigma or a conditioning tensor that requires grad is refused with NotImplementedError."""
        self._refuse_when_dropping("forward")
        if _wants_input_grad(x):
            return _InputGrad.apply(x, self, sigma, aug_cond, class_cond, mapping_cond, None)
        return self._run(x, sigma, aug_cond, class_cond, mapping_cond, None)

    def forward_preconditioned(self, x, sigma, sigma_data, aug_cond=None, class_cond=None, mapping_cond=None):
        """Denoiser D(x, sigma) = F(x * c_in, sigma) * c_out + x * c_skip (k_diffusion/layers.py:88-90)
        with c_in folded into the patch gather and c_out / c_skip into the un-patch scatter.  Differentiable w.r.t. x as ``forward``."""
        self._refuse_when_dropping("forward_preconditioned")
        if _wants_input_grad(x):
            return _InputGrad.apply(x, self, sigma, aug_cond, class_cond, mapping_cond, sigma_data)
        return self._run(x, sigma, aug_cond, class_cond, mapping_cond, sigma_data)

    def forward_jvp(self, x, sigma, x_dot, aug_cond=None, class_cond=None, mapping_cond=None, sigma_data=None):
        """Dual pass (forward-mode JVP, models/jvp.py): (F(x, sigma), J_F x_dot) with the conditioning held fixed, or with ``sigma_data``
        the same for the Karras denoiser D(x) = F(x c_in) c_out + x c_skip.  fp32 in every arithmetic mode; no launch plan involved."""
        self._refuse_when_dropping("forward_jvp")
        from . import jvp
        return jvp.forward_jvp(self, x, sigma, x_dot, aug_cond=aug_cond, class_cond=class_cond, mapping_cond=mapping_cond, sigma_data=sigma_data)

    def _check_input(self, x, class_cond, mapping_cond, subject, other=None):
        """The input contract of every pass -> (x, other tensor or None), contiguous: the conditioning this model needs is given, x is
        [B, in_channels, H, W] fp32 on a ROCm device.  ``subject`` names the pass in the no-CPU-fallback error.  ``other``: (tensor,
        channels, message) of the pass's second tensor (tangent, output gradient), checked to be [B, channels, H, W] fp32 on a ROCm
        device as well; ``message`` formats (its shape, the expected shape)."""
        if class_cond is None and self.class_emb is not None:
            raise ValueError("class_cond must be specified if num_classes > 0")
        if mapping_cond is None and self.mapping_cond_in_proj is not None:
            raise ValueError("mapping_cond must be specified if mapping_cond_dim > 0")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"expected input [B, {self.in_channels}, H, W], got {tuple(x.shape)}")
        ts = (x,)
        if other is not None:
            t, channels, message = other
            shape = (x.shape[0], channels, *x.shape[2:])
            if tuple(t.shape) != shape:
                raise ValueError(message.format(tuple(t.shape), shape))
            ts = (x, t)
        if not all(t.is_cuda for t in ts):
            raise RuntimeError(f"{subject} runs on the HIP path only: move the model and inputs to a ROCm device (there is no CPU fallback)")
        if any(t.dtype != torch.float32 for t in ts):
            raise TypeError(f"fp32 inputs only (got {', '.join(str(t.dtype) for t in ts)})")
        return x.contiguous(), None if other is None else ts[1].contiguous()

    def _token_grids(self, x):
        """Token grid (h, w) of every level for the input ``x``, which must be on the weights' device."""
        if self.patch_in.proj.weight.device != x.device:
            raise RuntimeError(f"model weights are on {self.patch_in.proj.weight.device}, input on {x.device}")
        H, W = x.shape[2:]
        ph, pw = self.patch_size
        if H % ph or W % pw:
            raise ValueError(f"input {H}x{W} not divisible by the patch size {ph}x{pw}")
        grids = [(H // ph, W // pw)]
        for _ in self.level_specs[1:]:
            gh, gw = grids[-1]
            if gh % 2 or gw % 2:
                raise ValueError(f"token grid {gh}x{gw} cannot be merged 2x2")
            grids.append((gh // 2, gw // 2))
        return grids

    @torch.no_grad()
    def _run(self, x, sigma, aug_cond, class_cond, mapping_cond, sigma_data):
        x, _ = self._check_input(x, class_cond, mapping_cond, "ImageTransformerDenoiserModelV2")
        B, _, H, W = x.shape
        plan = self._plan_for(x, aug_cond, class_cond, create=True)
        table = plan.tables.table_for(sigma, aug_cond, class_cond, mapping_cond)
        if sigma_data is not None:                # per-sample sigma of the preconditioning folded into patch-in / patch-out
            if sigma.numel() != B or sigma.dtype != torch.float32 or not sigma.is_contiguous() or sigma.device != x.device:
                plan.sigma.copy_(sigma.reshape(-1).expand(B) if sigma.numel() == 1 else sigma.reshape(B), non_blocking=True)
                plan.sigma_ptr = plan.sigma.data_ptr()
            else:
                plan.sigma_ptr = sigma.data_ptr()  # read in place: freed storage is not reused before this stream's work is done
        plan.tables.mark_entry()                  # everything before this step's main chain (incl. an inline conditioning chain)
        out = torch.empty(B, self.out_channels, H, W, device=x.device, dtype=torch.float32)
        plan.run(x, out, sigma_data, table)
        return out

    def _plan_for(self, x, aug_cond, class_cond, create):
        """The launch plan of this (batch, size, conditioning kinds, device, arithmetic mode) combination."""
        B, _, H, W = x.shape
        fp = self._weights_fingerprint()
        if fp != self._fingerprint:
            if not create:
                return None
            self._drop_plans()
            self._fingerprint, self._packed, self._derived = fp, {}, {}
        has_class = self.class_emb is not None
        # Kernel selection is fixed when a plan is built (route_layer): by the arithmetic mode, by the environment switches read here and by
        # library options (kd_ffn_f32_supported follows "ffn_x3").  The switches are part of the key; a change of any library option
        # (nat.option_epoch, bumped by set_option and by a changed KDIFF_OPTIONS / KDIFF_* variable) drops the cached plans, so an
        # A/B run on ONE model object really compares two plans.
        nat.lib()                                  # (syncs the environment-mapped options -> option_epoch)
        if self._plans_epoch != nat.option_epoch:
            if not create:
                return None
            self._drop_plans()
            self._plans_epoch = nat.option_epoch
        key = (B, H, W, aug_cond is not None, has_class, self.mapping_cond_in_proj is not None, x.device, nat.default_precision()) \
            + tuple(os.environ.get(k, d) for k, d in PLAN_SWITCHES)
        plan = self._plan_cache.get(key)
        if plan is None and create:
            grids = self._token_grids(x)

            def build():
                with torch.inference_mode(False):     # (workspaces made under inference_mode could not be written in place outside it later)
                    return _Plan(self, B, H, W, grids, key[3], has_class, key[5], x.device, key[7],
                                 dict(zip((name for name, _ in PLAN_SWITCHES), key[8:])))
            # a plan owns the workspaces of its shape (~20 MB per 256 x 256 image in the fp32 modes): a caller that walks through batch
            # sizes would otherwise keep them all.  With MAX_PLANS shapes cached the least recently used one goes first, behind a wait
            # for its whole device (rare: only when a NEW shape arrives then).
            plan = self._plan_cache.put(key, build, MAX_PLANS)
        if plan is not None and has_class and class_cond is not None:
            # nn.Embedding raises on an out-of-range id (on every call); the HIP kernel would read past the table.  Checked whenever
            # the ids are a tensor this plan has not seen in this state (address, version): one device->host read per new id
            # tensor -- a sampling run passes the same tensor to every step, so the per-step path stays sync-free.
            # (tensors made under torch.inference_mode() carry no version counter: they cannot be recognised as unchanged and are
            # re-checked on every call.  A few identities are remembered, so alternating id tensors -- cond / uncond calls of a
            # guidance wrapper -- stay sync-free as well.)
            ident = weights.ident(class_cond)
            if ident not in plan.class_checked:
                lo, hi = (int(class_cond.min()), int(class_cond.max())) if class_cond.numel() else (0, 0)
                if lo < 0 or hi >= self.class_emb.weight.shape[0]:
                    raise IndexError(f"class_cond ids must lie in [0, {self.class_emb.weight.shape[0] - 1}] (got {lo}..{hi})")
                if not class_cond.is_inference():
                    plan.class_checked[ident] = class_cond        # (kept alive: the address cannot be recycled under the record)
                    while len(plan.class_checked) > CLASS_IDS_KEPT:
                        del plan.class_checked[next(iter(plan.class_checked))]
        return plan

    # ---- conditioning ahead of time ---------------------------------------------------------------
    def _hint_usable(self, x_like, class_cond, mapping_cond):
        if not x_like.is_cuda or x_like.dim() != 4:
            return False
        return not ((class_cond is None and self.class_emb is not None) or (mapping_cond is None and self.mapping_cond_in_proj is not None))

    @torch.no_grad()
    def prefetch_schedule(self, x_like, sigma_table, aug_cond=None, class_cond=None, mapping_cond=None):
        """Hint from the solver loop: model calls of this run will pass ROWS of ``sigma_table`` ([n, B] fp32 on the device,
        one row per call) as their sigma, together with exactly these other conditioning tensors.  The conditioning chain
        depends on sigma / class / aug / mapping_cond only, never on x, so it runs here once for all n x B rows (the same
        row-by-row kernels as the per-step chain: bit-identical scales) and every such call finds its [B, scale_width]
        table ready.  Calls that pass anything else fall back to the per-step chain.  Returns True when taken."""
        if not self._hint_usable(x_like, class_cond, mapping_cond) or sigma_table.dim() != 2 or not sigma_table.is_cuda:
            return False
        n, B = sigma_table.shape
        if B != x_like.shape[0] or n == 0 or sigma_table.dtype != torch.float32 or not sigma_table.is_contiguous():
            return False
        plan = self._plan_for(x_like, aug_cond, class_cond, create=True)
        return plan.tables.hint_schedule(sigma_table, aug_cond, class_cond, mapping_cond)

    def release_schedules(self):
        """Drop the scale tables (and the hinted tensors they keep alive) of finished runs: up to SCHEDULE_TABLE_MAX_BYTES of HBM
        per plan otherwise stay allocated until the next run replaces them.  Safe at any time: calls no table covers use the
        per-step chain, with the same bits."""
        for plan in self._plans.values():
            plan.tables.release()

    @torch.no_grad()
    def prefetch_conditioning(self, x_like, sigma, aug_cond=None, class_cond=None, mapping_cond=None):
        """Hint from the solver loop: the NEXT model call will use exactly these conditioning tensors.  Unless a schedule
        hint already covers that call, the conditioning chain then runs on a side HIP stream, concurrently with the main
        chain of the step in flight, into the other scale table; the next ``forward`` with the same tensors just waits for
        its event.  A hint that is not followed costs nothing but the side-stream work."""
        if not self._hint_usable(x_like, class_cond, mapping_cond):
            return
        plan = self._plan_for(x_like, aug_cond, class_cond, create=False)
        if plan is not None:
            plan.tables.hint_next(sigma, aug_cond, class_cond, mapping_cond)

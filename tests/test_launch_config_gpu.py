"""Every launch configuration the host dispatch can choose, forced through kd_set_option and run through the guard-band protocol.

The dispatch picks n-splits, tile forms, wave counts and slices from the shape and the CU count; a test at a few hundred rows gets whatever the
cost model returns there.  Each row of the tables below forces ONE configuration (``KDIFF_OPTIONS`` names, README), runs the op on guarded
tensors (tests/guard.py: ``run_case``), asserts from the launch profile that a launch of the expected kernel WITH the expected `` cfg=`` field
served it (the field states what was launched, not what was asked for), and compares with the fp64 / oracle reference at the tolerance the
op's existing test states -- the builders of tests/test_bounds_gpu.py cite them; a forced configuration of the same arithmetic is the same
arithmetic, so no new tolerance appears here.  Where only the assignment of n-tiles to workgroups changes (n-splits) the result must also be
the same bits as the default configuration's at that shape: a tile's K loop does not depend on which workgroup runs it.

AUTO: configurations the dispatch reaches by itself at some shape / CU count (they matter most and run first).  REQUEST: variants compiled
in and documented but reachable only through an option, the plain "off" switches (which kernel serves the shape instead) and the thresholds
(one shape below, one at the moved threshold).  PLAN_ROWS: the switches and thresholds that act through a ``*_supported`` predicate of the C ABI, which
the model's launch plan asks (kd_gemm_mx8 and the block entry points also refuse what their predicate refuses; kd_ffn_bf16 / kd_ffn_f32 launch
whatever they are handed): a forward of a small model per row, the plan's launch names, the kernels in the profile, and the CPU oracle.  PREDICATES:
the same switches at the predicate itself; tests/test_launch_config_cpu.py runs them, no launch is involved.

The tables are built at import and need no GPU (tests/test_launch_config_cpu.py reads them); the tests do.
"""
import re

import pytest
import torch

from k_diffusion_amd import _native as nat
from tests import test_bounds_gpu as tb
from tests.guard import run_case, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
RESET = -2 ** 31                      # kd_set_option: back to the built-in default
E_STORE, E_RES, E_GEGLU, E_QKV = nat.EPI_STORE, nat.EPI_RESIDUAL, nat.EPI_GEGLU, nat.EPI_QKV


# ---- the `` cfg=`` matcher ---------------------------------------------------------------------------------------------------------------------

def cfg_of(name):
    """The configuration field of a launch-profile name (None: the launch site states none)."""
    m = re.search(r" cfg=(\S+)", name)
    return m.group(1) if m else None


def served(names, kernel, cfg):
    """Did a launch whose name starts with ``kernel`` AND carries ``cfg`` (None: any) serve the call?  The kernel prefix alone is not enough:
    the same kernel under another configuration is exactly what a row must not mistake for its own."""
    names = [n.replace(", ", ",") for n in names]
    return any(n.startswith(kernel) and (cfg is None or cfg_of(n) == cfg) for n in names)


def assert_served(what, names, kernel, cfg):
    assert served(names, kernel, cfg), (f"{what}: expected a launch of {kernel}* with cfg={cfg}, the profile has "
                                        f"{sorted({n.replace(', ', ',') for n in names})}: the row tested nothing")


# ---- host rules restated (the expected configuration where an option leaves part of the choice to the dispatch) ------------------------------------

def best_n_splits(panels, n_tiles, slots, prologue_weight):
    """kd_common.h: best_n_splits (the split3, bf16 and fp8 a-stationary launchers all call it; bf16 with weight 1)"""
    best, best_cost = 1, None
    for sp in range(1, n_tiles + 1):
        if n_tiles % sp:
            continue
        cost = -(-panels * sp // slots) * (prologue_weight + n_tiles // sp)
        if best_cost is None or cost < best_cost:
            best, best_cost = sp, cost
    return best


def tiled_cfg(M, N, K, bm=0, lw=1):
    """gemm_bf16.hip: gemm_tiled_try.  The loader-wave form needs 128-row tiles, at most one tile per CU and K >= 768, and runs on the deep ring."""
    def f(cus):
        t128, t256 = -(-M // 128) * -(-N // 128), -(-M // 256) * -(-N // 128)
        big = bm == 256 if bm else t256 >= cus
        one_round = not big and t128 <= cus
        use_lw = bool(one_round and K >= 768 and lw)
        return f"bm{256 if big else 128},lw{int(use_lw)},deep{int(use_lw)}"
    return f


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------

class Row:
    """``case``: a tests/guard.py Case from a builder of tests/test_bounds_gpu.py; ``opts``: the options forced around it; ``kernel`` / ``cfg``: the
    launch that must have served it (cfg: a string, a function of the CU count, or None where the launch site states no configuration);
    ``bits``: the result must be the same bits as under the default configuration."""

    def __init__(self, case, opts, kernel, cfg=None, bits=False):
        self.case, self.opts, self.kernel, self.cfg, self.bits = case, dict(opts), kernel, cfg, bits
        self.mode = case.mode                  # KDIFF_GEMM for the fp32 ops (None: bf16 / fp8 tensors pick their own kernels)
        self.id = case.name + "|" + (",".join(f"{k}={v}" for k, v in self.opts.items()) or "default")

    def __repr__(self):
        return self.id


_CASES = {}


def built(builder, *args, pick="", **kw):
    """The one Case ``builder(*args, **kw)`` adds (of several: the one whose name starts with ``pick``), shared between the rows that use it."""
    got = []
    with tb.collect_into(got):
        builder(*args, **kw)
    got = [c for c in got if c.name.startswith(pick)]
    assert len(got) == 1, [c.name for c in got]
    return _CASES.setdefault(got[0].name, got[0])


# row counts: 1024 = 8 panels of 128 (panel_split's XCD branch), 1000 = 8 panels with a ragged last one, 768 = 6 panels (the plain branch),
# 1100 = 9 panels, ragged.  Token grids for the qkv epilogue (one sample); four samples for the per-sample scales, so that at 1000 and 1100 rows
# a 32-row block straddles two samples
GRID = {1024: (32, 32), 1000: (25, 40), 768: (24, 32), 1100: (25, 44), 2048: (32, 64)}
M4 = (1024, 1000, 768, 1100)


def lin(kind, M, N, K, mode, kernel, src, bf=False, B=4):
    return built(tb._lin, kind, M, N, K, mode, bf=bf, B=B, kernel=kernel, src=src)


def qkv(M, nh, K, mode, kernel, src, bf=False, packed=False):
    H, W = GRID[M]
    name = f"norm_linear[qkv{'_packed' if packed else ''},{'bf16' if bf else mode},{H}x{W},nh{nh},B1,K{K}]"
    return built(tb._qkv, name, H, W, nh, 1, K, mode, bf=bf, packed=packed, kernel=kernel, src=src)


def splits_rows(table, c, option, kernel, n_tiles, splits, fmt="splits{}", extra=None):
    """One row per forced split count.  Every count up to n_tiles is a supported configuration of the full-tile kernels: panel_split (kd_common.h; the
    split3, bf16 and fp8 kernels share it) hands split s the tiles [n_tiles s / S, n_tiles (s + 1) / S), which are disjoint, cover the range and are
    non-empty for S <= n_tiles, and a workgroup's loop takes its tile count from that range alone -- so non-divisors are rows like any other."""
    for sp in splits:
        assert 1 <= sp <= n_tiles
        table.append(Row(c, dict(extra or {}, **{option: sp}), kernel, fmt.format(sp), bits=True))


AUTO, REQUEST = [], []
X3, B16 = "gemm_x3.hip", "gemm_bf16.hip"

# -- gemm_x3_astat<e> (split3, full tiles): x3_splits.  K = 128 and K = 512 (K = 256 runs on half tiles by default: below, and REQUEST for x3_half=0)
for _M in M4:
    splits_rows(AUTO, lin("norm_ps", _M, 512, 128, "split3", "gemm_x3_astat", X3), "x3_splits", f"gemm_x3_astat<e{E_STORE}>", 4, (1, 2, 4, 3))
    splits_rows(AUTO, lin("norm_geglu_ps", _M, 384, 128, "split3", "gemm_x3_astat", X3), "x3_splits", f"gemm_x3_astat<e{E_GEGLU}>", 6, (1, 2, 3, 6, 4))
    splits_rows(AUTO, qkv(_M, 2, 128, "split3", "gemm_x3_astat<e5>", X3, packed=_M == 1000), "x3_splits", f"gemm_x3_astat<e{E_QKV}>", 3, (1, 3, 2))
    splits_rows(AUTO, qkv(_M, 8, 512, "split3", "gemm_x3_astat<e5>", X3), "x3_splits", f"gemm_x3_astat<e{E_QKV}>", 12, (1, 3, 12))
    splits_rows(AUTO, lin("norm_geglu_ps", _M, 768, 512, "split3", "gemm_x3_astat", X3), "x3_splits", f"gemm_x3_astat<e{E_GEGLU}>", 12, (1, 4, 12) + ((5,) if _M == 1100 else ()))

# -- gemm_x3_astat<e,h> (K = 256, half tiles, two workgroups per CU): x3_splits over the 12 half tiles; launch_half takes divisors only and
# answers any other request with the cost model's choice, which the cfg= field then states
for _M in M4:
    _panels = -(-_M // 128)
    for _c, _e in ((qkv(_M, 4, 256, "split3", "gemm_x3_astat<e5,h>", X3, packed=_M == 1100), E_QKV),
                   (lin("norm_geglu_ps", _M, 384, 256, "split3", "gemm_x3_astat", X3), E_GEGLU)):
        splits_rows(AUTO, _c, "x3_splits", f"gemm_x3_astat<e{_e},h>", 12, (1, 2, 3, 4, 6, 12))
        # (what runs IS the default configuration: the cfg= assertion is the row's content, a bit comparison would compare it with itself)
        AUTO.append(Row(_c, {"x3_splits": 5}, f"gemm_x3_astat<e{_e},h>", lambda cus, p=_panels: f"splits{best_n_splits(p, 12, 2 * cus, 2)}"))

# -- gemm_bf16_astat<e>: astat_splits (first / middle / last divisor and one non-divisor), K = 256 and 512
for _M in (1024, 1000, 768):
    for _K in (256, 512):
        _nq = 3 * _K // 128
        splits_rows(AUTO, lin("norm_ps", _M, 512, _K, None, "gemm_bf16_astat", B16, bf=True), "astat_splits", f"gemm_bf16_astat<e{E_STORE}>", 4, (1, 2, 4, 3), "rows128,splits{}")
        splits_rows(AUTO, qkv(_M, _K // 64, _K, None, "gemm_bf16_astat<e5>", B16, bf=True), "astat_splits", f"gemm_bf16_astat<e{E_QKV}>", _nq, (1, 3, _nq), "rows128,splits{}")
        splits_rows(AUTO, lin("norm_geglu_ps", _M, 384, _K, None, "gemm_bf16_astat", B16, bf=True), "astat_splits", f"gemm_bf16_astat<e{E_GEGLU}>", 6, (1, 2, 6, 4), "rows128,splits{}")

# -- gemm_mx8_astat (fp8 products): mx8_splits; the reference is test_gemm_mx8_vs_the_restated_arithmetic's (the builders restate it).
# (B, T) = (2, 512): 8 panels; (1, 1000): 8 panels, ragged; (3, 256): 6 panels
for _B, _T, _K in [(2, 512, 256), (1, 1000, 256), (3, 256, 512)]:
    _nt = 2 * _K // 128
    splits_rows(AUTO, built(tb._mx8, _B, _T, _K, 384, "store"), "mx8_splits", f"gemm_mx8_astat<e{E_STORE}>", _nt, (1, 2, _nt, 3))
    splits_rows(AUTO, built(tb._mx8, _B, _T, _K, 384, "geglu"), "mx8_splits", f"gemm_mx8_astat<e{E_GEGLU}>", 6, (1, 3, 6, 4))
    splits_rows(AUTO, built(tb._mx8_qkv, _B, _T, _K, 384), "mx8_splits", f"gemm_mx8_astat<e{E_QKV}>", 3 * _K // 128, (1, 2, 3 * _K // 128, 5))

# -- gemm_bf16_tiled<a,e>: tiled_bm x tiled_lw.  256-row tiles are the default only from cu_count() tiles on, i.e. at row counts that are multiples
# of 4096 in the model tests: 300 and 520 rows give them a ragged last tile, 1024 an exact one.  K = 1536 admits the loader-wave form.  The tile form
# changes which rows share a workgroup, not a row's K loop -- but that is not the n-tile assignment, so the reference bound stands alone here.
for _M, (_B, _h, _w) in ((300, (3, 10, 10)), (520, (2, 13, 20)), (1024, (1, 32, 32))):
    for _K in (256, 1536):
        # tiled_lw acts on 128-row tiles at K >= 768 only: no rows for the combinations where it changes nothing
        for _o in [{"tiled_bm": 128}, {"tiled_bm": 256}] if _K == 256 else [{"tiled_bm": 128, "tiled_lw": 0}, {"tiled_bm": 128, "tiled_lw": 1}, {"tiled_bm": 256}]:
            _cfg = tiled_cfg(_M, 256, _K, _o["tiled_bm"], _o.get("tiled_lw", 1))
            AUTO.append(Row(lin("plain", _M, 256, _K, None, None, None, bf=True), _o, f"gemm_bf16_tiled<a0,e{E_STORE}>", _cfg))
            AUTO.append(Row(lin("res", _M, 256, _K, None, None, None, bf=True), _o, f"gemm_bf16_tiled<a0,e{E_RES}>", _cfg))
            AUTO.append(Row(built(tb._merge_split, _B, _h, _w, 256, _K // 4, None, bf=True, pick="token_merge"), _o, f"gemm_bf16_tiled<a1,e{E_STORE}>", _cfg))
# 128-row tiles in more than one round of the chip (33 x 8 = 264 tiles, the last row tile ragged): no loader waves whatever tiled_lw says; and 256-row
# tiles of the same shapes (17 x 8, the last one with 104 rows)
for _o in ({"tiled_bm": 128, "tiled_lw": 1}, {"tiled_bm": 256}):
    AUTO.append(Row(lin("plain", 4200, 1024, 1536, None, None, None, bf=True), _o, f"gemm_bf16_tiled<a0,e{E_STORE}>", tiled_cfg(4200, 1024, 1536, _o["tiled_bm"], 1)))
    AUTO.append(Row(lin("res", 4200, 1024, 256, None, None, None, bf=True), _o, f"gemm_bf16_tiled<a0,e{E_RES}>", tiled_cfg(4200, 1024, 256, _o["tiled_bm"], 1)))

# -- gemm_bf16_wstat<e,n>: slices, forced by the shape (n_tiles > 144 KiB / (K / 64 blocks of 16 KiB): 4 tiles at K = 128, 2 at 256, 1 at 512).  At K = 256
# and 512 the dispatch reaches this kernel behind a norm where N is no multiple of the a-stationary kernel's tile.  N = 640 / 320 (GEGLU) / 288: a last slice
# shorter than the others; 288 also ends in a 32-column tile.  No other slicing exists at a shape (the slice count follows from N), so there is no default
# configuration to compare bits with: the reference bound stands alone.
for _M in (2048, 2075):
    AUTO.append(Row(lin("plain", _M, 512, 128, None, None, None, bf=True), {}, f"gemm_bf16_wstat<e{E_STORE},n0>", "waves8,pf0,slices1"))
    AUTO.append(Row(lin("plain", _M, 640, 128, None, None, None, bf=True), {}, f"gemm_bf16_wstat<e{E_STORE},n0>", "waves8,pf0,slices2"))
    AUTO.append(Row(lin("res", _M, 640, 128, None, None, None, bf=True), {}, f"gemm_bf16_wstat<e{E_RES},n0>", "waves8,pf0,slices2"))
for _M, _B in ((2048, 4), (2080, 5)):           # behind a norm a 32-row chunk is one sample's: 5 samples of 416 rows = 16 panels and a quarter
    AUTO.append(Row(lin("norm_geglu_ps", _M, 320, 128, None, "gemm_bf16_wstat", B16, bf=True, B=_B), {}, f"gemm_bf16_wstat<e{E_GEGLU},n1>", "waves8,pf0,slices2"))
    AUTO.append(Row(lin("norm_ps", _M, 160, 256, None, "gemm_bf16_wstat", B16, bf=True, B=_B), {}, f"gemm_bf16_wstat<e{E_STORE},n1>", "waves8,pf0,slices1"))
    AUTO.append(Row(lin("norm_ps", _M, 288, 256, None, "gemm_bf16_wstat", B16, bf=True, B=_B), {}, f"gemm_bf16_wstat<e{E_STORE},n1>", "waves8,pf0,slices2"))
    AUTO.append(Row(lin("norm_ps", _M, 96, 512, None, "gemm_bf16_wstat", B16, bf=True, B=_B), {}, f"gemm_bf16_wstat<e{E_STORE},n1>", "waves8,pf0,slices1"))
    AUTO.append(Row(lin("norm_ps", _M, 288, 512, None, "gemm_bf16_wstat", B16, bf=True, B=_B), {}, f"gemm_bf16_wstat<e{E_STORE},n1>", "waves8,pf0,slices3"))

# ---- request-only variants ------------------------------------------------------------------------------------------------------------------------
_plain_ws = lin("plain", 2075, 640, 128, None, None, None, bf=True)
_astat_b = lin("norm_ps", 1000, 512, 256, None, "gemm_bf16_astat", B16, bf=True)
_x3_store = lin("norm", 1000, 512, 128, "split3", "gemm_x3_astat", X3)
_qkv_256 = qkv(1000, 4, 256, "split3", "gemm_x3_astat<e5,h>", X3)
_geglu_256 = lin("norm_geglu_ps", 1100, 384, 256, "split3", "gemm_x3_astat", X3)
REQUEST += [
    Row(_plain_ws, {"wstat_max_slices": 1}, f"gemm_bf16_tiled<a0,e{E_STORE}>"),                # two slices refused: the tiled kernel serves the shape
    # the fused feed-forward forms
    Row(built(tb._ffn, "ffn[split3,30x30,B3,K128,dff192]", (3, 30, 30), 128, 192, False, kernel="ffn_x3"), {"ffn_x3_half": 0}, "ffn_x3 ", "half0"),
    Row(built(tb._ffn, "ffn[split3,25x44,B1,K128,dff384]", (1, 25, 44), 128, 384, False, kernel="ffn_x3"), {"ffn_x3_half": 0}, "ffn_x3 ", "half0"),
    # patch-in / patch-out without the 4 x 4 patch kernels
    Row(built(tb._patch, 3, 72, 88, 4, 128, None, bf=True, pick="patch_in"), {"patch_fast": 0}, f"gemm_bf16_generic<a2,e{E_STORE}>"),
    Row(built(tb._patch, 3, 72, 88, 4, 128, None, bf=True, pick="patch_out"), {"patch_fast": 0}, "gemm_bf16_generic<a0,e4>"),
    # K = 256 on full tiles (one workgroup per CU) instead of half tiles: 6 n-tiles.  (Another kernel than the default's, not another assignment
    # of its tiles: no bit comparison)
    Row(_qkv_256, {"x3_half": 0, "x3_splits": 3}, f"gemm_x3_astat<e{E_QKV}> ", "splits3"),
    Row(_qkv_256, {"x3_half": 0, "x3_splits": 4}, f"gemm_x3_astat<e{E_QKV}> ", "splits4"),
    Row(_geglu_256, {"x3_half": 0}, f"gemm_x3_astat<e{E_GEGLU}> ", lambda cus: f"splits{best_n_splits(9, 6, cus, 1)}"),
    # the round-1 a-stationary kernel (x3 = 0 leaves the shape to it) with the conservative store wait; 8 panels x 4 tiles -> 2 splits by its own rule
    Row(_x3_store, {"x3": 0, "astat_storewait": 1}, f"gemm_astat<e{E_STORE}>", "splits2,waves4"),
    Row(qkv(1024, 2, 128, "split3", "gemm_astat<e5>", "gemm_astat.hip"), {"x3": 0, "astat_storewait": 1}, f"gemm_astat<e{E_QKV}>", "splits1,waves4"),
    # the "off" switches: the default kernel of the shape first, then the kernel that serves it instead
    Row(lin("norm", 65, 8, 256, "exact", "gemm_skinny", "gemm_skinny.hip"), {}, f"gemm_skinny<n1,e{E_STORE}>"),
    Row(lin("norm", 65, 8, 256, "exact", "gemm_skinny", "gemm_skinny.hip"), {"skinny": 0}, f"gemm_f32<a0,n1,e{E_STORE}>"),
    Row(_x3_store, {"astat": 0}, f"gemm_bf16x3<a0,n1,e{E_STORE}>"),
    Row(lin("res", 300, 96, 512, "split3", None, None), {}, f"gemm_bf16x3<a0,n0,e{E_RES},ks2>"),
    Row(lin("res", 300, 96, 512, "split3", None, None), {"ksplit": 0}, f"gemm_bf16x3<a0,n0,e{E_RES}>"),
    Row(lin("plain", 2075, 96, 128, None, None, None, bf=True), {}, f"gemm_bf16_wstat<e{E_STORE},n0>", "waves8,pf0,slices1"),
    Row(lin("plain", 2075, 96, 128, None, None, None, bf=True), {"wstat": 0}, f"gemm_bf16_tiled<a0,e{E_STORE}>"),
    Row(lin("norm_ps", 2048, 512, 256, None, "gemm_bf16_astat", B16, bf=True), {}, f"gemm_bf16_astat<e{E_STORE}>"),
    Row(lin("norm_ps", 2048, 512, 256, None, "gemm_bf16_astat", B16, bf=True), {"astat_bf16": 0}, f"gemm_bf16_wstat<e{E_STORE},n1>", "waves8,pf0,slices2"),
    Row(_astat_b, {"astat_bf16": 0}, f"gemm_bf16_generic<a0,e{E_STORE}>"),          # 1000 rows: below the W-stationary kernel's 2048
    # thresholds, moved: one shape just below, one at the new value
    Row(lin("norm", 383, 512, 128, "split3", None, None), {"x3_min_rows": 384}, f"gemm_bf16x3<a0,n1,e{E_STORE}>"),
    Row(lin("norm", 384, 512, 128, "split3", "gemm_x3_astat", X3), {"x3_min_rows": 384}, f"gemm_x3_astat<e{E_STORE}>"),
    Row(lin("norm", 384, 512, 128, "split3", "gemm_x3_astat", X3), {}, f"gemm_bf16x3<a0,n1,e{E_STORE}>"),
    Row(lin("res", 63, 256, 256, "split3", None, None), {"x3r_min_rows": 64, "skinny": 0}, f"gemm_bf16x3<a0,n0,e{E_RES}"),
    Row(lin("res", 64, 256, 256, "split3", "gemm_x3r", "gemm_x3r.hip"), {"x3r_min_rows": 64, "skinny": 0}, f"gemm_x3r<a0,e{E_RES}>"),
    Row(lin("res", 64, 256, 256, "split3", "gemm_x3r", "gemm_x3r.hip"), {"skinny": 0}, f"gemm_bf16x3<a0,n0,e{E_RES}"),
    Row(lin("norm", 1000, 512, 512, "split3", None, None), {"x3": 0, "astat_max_k": 256}, f"gemm_bf16x3<a0,n1,e{E_STORE}>"),
    Row(lin("norm", 1000, 512, 512, "split3", None, None), {"x3": 0}, f"gemm_astat<e{E_STORE}>", "splits2,waves4"),
    Row(lin("norm", 1000, 512, 256, "split3", None, None), {"x3": 0, "astat_max_k": 256}, f"gemm_astat<e{E_STORE}>", "splits2,waves4"),
]

# the round-3 / round-4 split3 switches the README names (each also has an older test of its own, listed in tests/test_launch_config_cpu.py)
_res_x3r = lin("res", 1000, 256, 256, "split3", "gemm_x3r", "gemm_x3r.hip")
_att_pk = built(tb._attn, "attn_global", 8, 8, 2, 2, "split3", prep="packed", kernel="attn_global_x3")
REQUEST += [
    Row(_res_x3r, {}, f"gemm_x3r<a0,e{E_RES}>"),
    Row(_res_x3r, {"x3r_lw": 0}, f"gemm_x3r<a0,e{E_RES}>"),                       # (the form without loader waves: the same launch name)
    Row(_res_x3r, {"x3r": 0}, f"gemm_bf16x3<a0,n0,e{E_RES}"),
    Row(_att_pk, {}, "attn_global_x3"),
    Row(_att_pk, {"attn_x3": 0}, "attn_global_bf16x3"),
]

# ---- switches that act through a predicate of the C ABI: (options, predicate, arguments, answer by default, answer with the options) -------------------
# (kd_ffn_f32_supported at width 256 asks for 7/8 of the CUs in row panels by default: 3 or 4 panels never are)
PREDICATES = [
    ({"ffn_fused": 0}, "kd_ffn_bf16_supported", (16384, 128, 384), 1, 0),
    ({"ffn_bf16_min_rows": 1024}, "kd_ffn_bf16_supported", (1023, 128, 384), 0, 0),
    ({"ffn_bf16_min_rows": 1024}, "kd_ffn_bf16_supported", (1024, 128, 384), 0, 1),
    ({"ffn_x3": 0}, "kd_ffn_f32_supported", (2048, 128, 384), 1, 0),
    ({"ffn_x3_min_panels_256": 4}, "kd_ffn_f32_supported", (384, 256, 768), 0, 0),
    ({"ffn_x3_min_panels_256": 4}, "kd_ffn_f32_supported", (385, 256, 768), 0, 1),
    ({"attn_ffn_x3": 0}, "kd_attn_ffn_f32_supported", (2, 32, 32, 2, 7, 128, 384), 1, 0),
    ({"mx8": 0}, "kd_gemm_mx8_supported", (1024, 512, 256, E_STORE, 1), 1, 0),
    ({"proj_block_bf16": 0}, "kd_proj_block_bf16_supported", (256, 256, 384, E_GEGLU), 1, 0),
    ({"attn_block_bf16": 0}, "kd_attn_block_bf16_supported", (256, 256, 4), 1, 0),
]

# attention core: waves per workgroup of the dense kernel at 128 < T <= 256 (a ragged 208 and the full 256 tokens)
for _H, _Wd in ((13, 16), (16, 16)):
    _c = built(tb._attn, "attn_global", _H, _Wd, 2, 2, None, bf=True)
    REQUEST += [Row(_c, {}, "attn_global_bf16", "qw8"), Row(_c, {"attn_global_qw": 4}, "attn_global_bf16", "qw4"), Row(_c, {"attn_global_qw": 2}, "attn_global_bf16", "qw2")]


def forced_options():
    """Every option name a row sets around a launch (tests/test_launch_config_cpu.py: completeness)."""
    return {k for r in AUTO + REQUEST + PLAN_ROWS for k in r.opts}


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops(KD):
    return KD.ops


_DEFAULT = {}


def default_outputs(c, ops):
    """What the case's call returns with no option forced (computed once per case; the few-rows kernels are off as for every row)."""
    if c.name not in _DEFAULT:
        spec = c.make(ops)
        T = {k: v.to(DEV).clone() for k, v in spec["ins"].items()}
        T.update({k: torch.empty(shape, dtype=dt, device=DEV) for k, (shape, dt) in spec.get("outs", {}).items()})
        out = spec["call"](T)
        _DEFAULT[c.name] = [o.detach().cpu().clone() for o in (out if isinstance(out, (tuple, list)) else (out,))]
    return _DEFAULT[c.name]


def run_row(row, ops, monkeypatch):
    """One row: the default configuration's result first where bits are compared, then the options on (restored to the built-in defaults in
    ``finally``), the guard-band protocol under the launch profile, the served-by assertion and the bit comparison."""
    lib = nat.lib()
    if row.mode is not None:
        monkeypatch.setenv("KDIFF_GEMM", row.mode)
    opts = dict({"x3s_max_rows": 0, "b16s_max_rows": 0}, **row.opts)      # the few-rows kernels off, as in tests/test_bounds_gpu.py
    cfg = row.cfg(torch.cuda.get_device_properties(0).multi_processor_count) if callable(row.cfg) else row.cfg
    try:
        for k in ("x3s_max_rows", "b16s_max_rows"):
            nat.set_option(k, 0)
        base = default_outputs(row.case, ops) if row.bits else None
        for k, v in opts.items():
            nat.set_option(k, v)
        lib.kd_prof_reset()
        lib.kd_prof_enable(1)
        try:
            res = run_case(row.case, "nan", env=ops, device=DEV)
            names = tb._prof_names()
        finally:
            lib.kd_prof_enable(0)
            lib.kd_prof_reset()
    finally:
        for k in opts:
            nat.set_option(k, RESET)
    print(f"{row.id}: errors {['%.2e' % e for e in res.errs]}; launches {sorted({n.replace(', ', ',') for n in names})}")
    assert_served(row.id, names, row.kernel, cfg)
    if row.bits:
        assert len(base) == len(res.outputs)
        for i, (a, b) in enumerate(zip(res.outputs, base)):
            assert same_bits(a, b), f"{row.id}: result {i} differs from the default configuration's ({int((a != b).sum())} elements)"


def _params(table):
    ids = [r.id for r in table]
    assert len(ids) == len(set(ids)), "row ids are the test ids: unique"
    return [pytest.param(r, id=r.id) for r in table]


@pytest.mark.parametrize("row", _params(AUTO))
def test_auto_reachable_configurations(ops, row, monkeypatch):
    run_row(row, ops, monkeypatch)


@pytest.mark.parametrize("row", _params(REQUEST))
def test_request_only_configurations(ops, row, monkeypatch):
    run_row(row, ops, monkeypatch)


# ---- plan level: the switches and thresholds that act through the launch plan of the model ------------------------------------------------------------
# route_layer (models/image_transformer_v2.py) asks the library's ``*_supported`` predicates, which follow these options; kd_ffn_bf16 / kd_ffn_f32
# themselves launch whatever they are handed, so only a forward of a model shows which kernels serve a layer once a switch is off.  Each row: a small
# model, the arithmetic mode, the batch, the options, launch names (``_Launch.what``) the plan must / must not contain, profile-name prefixes that must /
# must not have run, and -- first -- names the DEFAULT plan of that model and batch must contain, i.e. the kernel the row switches off is what the
# default takes there.  The forward meets the CPU oracle at the bound of the existing whole-model oracle tests: 5e-4 in split3 mode
# (tests/test_model_gpu.py::test_unusual_shapes_vs_oracle), 2.5e-2 in bf16 mode (test_unusual_shapes_bf16).  fp8 mode with mx8=0 is the bf16 plan: held to
# the bf16 bound and to the bits of the bf16-mode forward (the default fp8 forward has its own gate in test_forward_fp8_mode and gets none here).
_G = {"type": "global", "d_head": 64}
PLAN_MODELS = {
    # level 0: 32 x 32 tokens, width 128, neighbourhood attention (2 048 rows at batch 2: the smallest the fused split3 kernels take); mid: 256 tokens, width 256
    "na128_g256": dict(input_size=[64, 64], depths=[1, 1], widths=[128, 256], d_ffs=[384, 768], self_attns=[{"type": "neighborhood", "d_head": 64, "kernel_size": 7}, _G]),
    "g128": dict(input_size=[32, 32], depths=[1], widths=[128], d_ffs=[256], self_attns=[_G]),          # 256 tokens per sample, width 128
    "g256": dict(input_size=[32, 32], depths=[1], widths=[256], d_ffs=[768], self_attns=[_G]),          # 256 tokens per sample, width 256
}
PLAN_BOUND = {"split3": 5e-4, "bf16": 2.5e-2, "fp8": 2.5e-2}


class PlanRow:
    def __init__(self, model, mode, batch, opts, default_has, has, lacks, ran, not_ran, same_as_bf16=False):
        self.model, self.mode, self.batch, self.opts, self.default_has, self.has, self.lacks = model, mode, batch, dict(opts), default_has, has, lacks
        self.ran, self.not_ran, self.same_as_bf16 = ran, not_ran, same_as_bf16
        self.id = f"{model},{mode},B{batch}|" + ",".join(f"{k}={v}" for k, v in self.opts.items())


_L0, _MID = "down_levels.0.0.", "mid_level.0."
PLAN_ROWS = [
    # split3, level 0: core + out projection + FF in one launch by default
    PlanRow("na128_g256", "split3", 2, {"attn_ffn_x3": 0}, [_L0 + "attn_na2d+ff", "up_levels.0.0.attn_na2d+ff"], [_L0 + "attn_na2d", _L0 + "ff", "up_levels.0.0.ff"],
            ["+ff", _L0 + "out_proj"], ["attn_na2d_x3", "ffn_x3+out"], ["attn_ffn_x3"]),
    PlanRow("na128_g256", "split3", 2, {"ffn_x3": 0}, [_L0 + "attn_na2d+ff"], [_L0 + "attn_na2d", _L0 + "out_proj", _L0 + "up_proj", _L0 + "down_proj", "up_levels.0.0.up_proj"],
            ["+ff", ".ff"], [(f"gemm_x3_astat<e{E_GEGLU}>", f"gemm_x3s<n1,e{E_GEGLU}>")], ["attn_ffn_x3", "ffn_x3"]),
    # split3, width 256: the fused FF block from ffn_x3_min_panels_256 row panels on (default: 7/8 of the CUs); the mid level has 4 at batch 2
    PlanRow("na128_g256", "split3", 2, {"ffn_x3_min_panels_256": 4}, [_MID + "up_proj", _MID + "down_proj"], [_MID + "ff"], [_MID + "up_proj", _MID + "out_proj"], ["ffn_x3+out M=512 K=256"], []),
    PlanRow("na128_g256", "split3", 2, {"ffn_x3_min_panels_256": 5}, [_MID + "up_proj"], [_MID + "up_proj", _MID + "down_proj", _MID + "out_proj"], [_MID + "ff"], [], ["ffn_x3+out M=512 K=256", "ffn_x3 M=512 K=256"]),
    # bf16, width 128: the fused FF block from ffn_bf16_min_rows = 16 384 rows on (batch 64 x 256 tokens)
    PlanRow("g128", "bf16", 64, {"ffn_fused": 0}, [_MID + "ff"], [_MID + "up_proj", _MID + "down_proj", _MID + "out_proj"], [".ff"], ["gemm_bf16_wstat<e2,n1>"], ["ffn_bf16"]),
    PlanRow("g128", "bf16", 8, {"ffn_bf16_min_rows": 2048}, [_MID + "up_proj", _MID + "down_proj"], [_MID + "ff"], [_MID + "up_proj", _MID + "out_proj"], ["ffn_bf16+out M=2048"], []),
    PlanRow("g128", "bf16", 8, {"ffn_bf16_min_rows": 2049}, [_MID + "up_proj"], [_MID + "up_proj", _MID + "down_proj", _MID + "out_proj"], [".ff"], [], ["ffn_bf16"]),
    # bf16, width 256, 256 tokens per sample, 48 samples: the one-launch attention block and the block form of the up projection (192 workgroups)
    PlanRow("g256", "bf16", 48, {"attn_block_bf16": 0}, [_MID + "attn_block"], [_MID + "qkv_proj", _MID + "attn_global"], [_MID + "attn_block"],
            [f"gemm_bf16_astat<e{E_QKV}>", "attn_global_bf16"], ["attn_block_bf16"]),
    PlanRow("g256", "bf16", 48, {"proj_block_bf16": 0}, [_MID + "up_proj(block)"], [_MID + "up_proj", _MID + "attn_block"], [_MID + "up_proj(block)"],
            [f"gemm_bf16_astat<e{E_GEGLU}>"], ["proj_block_bf16"]),
    # fp8 mode: the up / down projections on the fp8 matrix instruction (12 288 rows >= mx8_min_rows); without them the plan is the bf16 mode's
    PlanRow("g256", "fp8", 48, {"mx8": 0}, [_MID + "up_proj(mx8)", _MID + "down_proj(mx8)"], [_MID + "up_proj(block)", _MID + "down_proj"], ["(mx8)"],
            ["proj_block_bf16"], ["gemm_mx8"], same_as_bf16=True),
]

_PLAN_STATE = {}


def _plan_model(KD, name):
    """(config, model on the GPU, its weights on the CPU), built once."""
    if ("model", name) not in _PLAN_STATE:
        raw = {"model": dict(PLAN_MODELS[name], type="image_transformer_v2", input_channels=2, patch_size=[2, 2], sigma_data=0.7, sigma_min=1e-2, sigma_max=50),
               "dataset": {"num_classes": 5}}
        cfg = KD.config.load_config(raw)
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        sd = KD.synth.synth_state_dict(model.state_dict(), seed=21)
        model.load_state_dict(sd)
        _PLAN_STATE["model", name] = (cfg, model.to(DEV), sd)
    return _PLAN_STATE["model", name]


def _plan_inputs(cfg, batch):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(batch, 2, *cfg["model"]["input_size"], generator=g) * 2
    return x, torch.tensor([0.05, 1.3, 20.0]).repeat(-(-batch // 3))[:batch], torch.arange(batch) % 6


def _plan_reference(KD, name, batch):
    """The CPU oracle's forward (computed once per model and batch, shared by the rows)."""
    from oracle import hdit
    if ("ref", name, batch) not in _PLAN_STATE:
        cfg, _, sd = _plan_model(KD, name)
        x, sigma, cls = _plan_inputs(cfg, batch)
        _PLAN_STATE["ref", name, batch] = hdit.forward(sd, cfg["model"], x, sigma, class_cond=cls)
    return _PLAN_STATE["ref", name, batch]


def _forward(KD, name, batch):
    """One forward under the launch profile -> (output on the CPU, the plan's launch names without the conditioning chain's, profile names)."""
    cfg, model, _ = _plan_model(KD, name)
    x, sigma, cls = _plan_inputs(cfg, batch)
    lib = nat.lib()
    lib.kd_prof_reset()
    lib.kd_prof_enable(1)
    try:
        y = model(x.to(DEV), sigma.to(DEV), class_cond=cls.to(DEV)).float().cpu()
        torch.cuda.synchronize()
        names = [n.replace(", ", ",") for n in tb._prof_names()]
    finally:
        lib.kd_prof_enable(0)
        lib.kd_prof_reset()
    whats = [ln.what for ln in list(model._plans.values())[-1].launches if not ln.what.startswith("mapping")]
    return y, whats, names


def _contains(whats, pat):
    """An exact launch name (patterns with a layer prefix) or, for the others, a suffix of any"""
    return pat in whats if pat.startswith(("down_levels", "up_levels", "mid_level")) else any(w.endswith(pat) for w in whats)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in PLAN_ROWS])
def test_plan_level_switches(KD, row, monkeypatch):
    from tests.helpers import relerr
    monkeypatch.setenv("KDIFF_GEMM", row.mode)
    ref = _plan_reference(KD, row.model, row.batch)
    y0, whats0, names0 = _forward(KD, row.model, row.batch)                  # the default plan takes what the row switches off
    for pat in row.default_has:
        assert _contains(whats0, pat), f"{row.id}: the default plan has no launch {pat}: {whats0}"
    if row.mode != "fp8":
        e0 = relerr(y0, ref)
        assert e0 < PLAN_BOUND[row.mode], f"{row.id}: default forward {e0:.3e} from the oracle"
    try:
        for k, v in row.opts.items():
            nat.set_option(k, v)
        y, whats, names = _forward(KD, row.model, row.batch)
    finally:
        for k in row.opts:
            nat.set_option(k, RESET)
    err = relerr(y, ref)
    print(f"{row.id}: error {err:.3e} (bound {PLAN_BOUND[row.mode]:.1e}); plan {whats}; kernels {sorted({n.split(' ')[0] for n in names})}")
    for pat in row.has:
        assert _contains(whats, pat), f"{row.id}: the plan has no launch {pat}: {whats}"
    for pat in row.lacks:
        assert not _contains(whats, pat), f"{row.id}: the plan still has a launch {pat}: {whats}"
    for pre in row.ran:
        assert any(n.startswith(pre) for n in names), f"{row.id}: no launch of {pre}* in the profile: {sorted(set(names))}"
    for pre in row.not_ran:
        assert not any(n.startswith(pre) for n in names), f"{row.id}: {pre}* still ran: {sorted(set(names))}"
    assert err < PLAN_BOUND[row.mode], f"{row.id}: {err:.3e} from the oracle, bound {PLAN_BOUND[row.mode]:.1e}"
    if row.same_as_bf16:
        monkeypatch.setenv("KDIFF_GEMM", "bf16")
        yb, _, _ = _forward(KD, row.model, row.batch)
        assert torch.equal(y, yb), f"{row.id}: differs from the bf16-mode forward, whose plan it is"

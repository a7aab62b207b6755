"""Completeness of tests/test_launch_config_gpu.py, without a GPU: every option the dispatch code reads (``opt(KD_OPT_name)``) is forced by a row of
that file's tables, set around a kernel launch by a named existing GPU test, or exempt because it selects no arithmetic path -- an option added
later without a row fails here.  Also: the rows name registered options only, the `` cfg=`` matcher refuses the right kernel under another
configuration (fake ops on the CPU, as tests/test_guard_cpu.py does for the guard protocol), and the switches that act through a
``*_supported`` predicate of the C ABI flip it (what the model's plan then launches: PLAN_ROWS of the GPU file)."""
import ast
import os
import re

import pytest
import torch

from k_diffusion_amd import _native as nat
from tests import test_launch_config_gpu as lc
from tests.guard import Case, run_case
from tests.helpers import source_options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# options already set around a kernel launch by an existing GPU test: name -> (file, test).  (The option-table and environment-plumbing checks of
# tests/test_host_cpu.py do not count: they launch nothing.)
EXISTING = {
    "x3s_max_rows": ("tests/test_ops_gpu.py", "test_split3_few_rows_latency_kernel"),
    "x3s_max_wgs": ("tests/test_ops_gpu.py", "test_split3_few_rows_latency_kernel"),
    "b16s_max_rows": ("tests/test_ops_gpu.py", "test_bf16_few_rows_latency_kernel"),
    "b16s_max_wgs": ("tests/test_ops_gpu.py", "test_bf16_few_rows_latency_kernel"),
    "ffn_fused_256": ("tests/test_ops_gpu.py", "test_bf16_fused_ffn_width_256"),
    "attn_x3": ("tests/test_ops_gpu.py", "test_split_stored_qkv_feeds_the_attention_cores"),
    "x3r_split": ("tests/test_ops_gpu.py", "test_token_split_multi_tile"),
    "x3_unpatch": ("tests/test_ops_gpu.py", "test_split3_patch_out_round3"),
    "x3_res": ("tests/test_ops_gpu.py", "test_split3_residual_projection_round3"),
    "x3r": ("tests/test_ops_gpu.py", "test_split3_residual_projection_round3"),
    "x3r_lw": ("tests/test_ops_gpu.py", "test_split3_residual_projection_round3"),
    "bf16_fast": ("tests/test_model_gpu.py", "test_forward_bf16_vs_reference"),
}
# options that select no arithmetic path
EXEMPT = {
    "code_warm": "how many workgroups pre-read the kernel's code into the L2; tests/test_model_gpu.py shows it changes no result",
    "gemm_debug": "benchmarks/ only: removes stores / MFMAs / erf for timing ablations, the results are not the op's",
}


def _test_source(path, test):
    text = open(os.path.join(REPO, path)).read()
    for node in ast.parse(text).body:
        if isinstance(node, ast.FunctionDef) and node.name == test:
            return ast.get_source_segment(text, node)
    return None


def test_every_option_is_forced_by_a_row_or_accounted_for():
    names = source_options()
    assert {"x3_splits", "astat_splits", "mx8_splits", "tiled_bm", "attn_global_qw"} <= names
    forced = lc.forced_options()
    unaccounted = sorted(n for n in names if n not in forced and n not in EXISTING and n not in EXEMPT)
    assert not unaccounted, f"options no test forces around a launch (add a row to tests/test_launch_config_gpu.py): {unaccounted}"
    stale = sorted((set(EXISTING) | set(EXEMPT)) - names)
    assert not stale, f"entries for options the sources no longer read: {stale}"
    assert not set(EXEMPT) & (forced | set(EXISTING))
    assert set(EXEMPT) == {"code_warm", "gemm_debug"}          # the list does not grow quietly
    for name, (path, test) in EXISTING.items():
        src = _test_source(path, test)
        assert src is not None, f"{path}::{test} does not exist"
        assert re.search(r'set_option\(\s*"%s"|KDIFF_OPTIONS.*\b%s=|\("%s", ' % (name, name, name), src), f"{path}::{test} does not set {name!r}"
        assert "pytest.mark.gpu" in open(os.path.join(REPO, path)).read()


def test_rows_force_registered_options_only():
    names = source_options()          # (tests/test_host_cpu.py: every one of them is in the library's table)
    for row in lc.PLAN_ROWS:
        assert row.opts and set(row.opts) <= names and row.mode in lc.PLAN_BOUND and row.model in lc.PLAN_MODELS and row.default_has, row.id
    # every switch the predicate table knows is also forced around a forward
    assert {k for o, *_ in lc.PREDICATES for k in o} <= {k for r in lc.PLAN_ROWS for k in r.opts}
    for row in lc.AUTO + lc.REQUEST:
        assert set(row.opts) <= names, (row.id, sorted(set(row.opts) - names))
        assert row.kernel and (row.cfg is None or callable(row.cfg) or re.fullmatch(r"[a-z0-9,]+", row.cfg)), row.id
        if callable(row.cfg):
            assert all(re.fullmatch(r"[a-z0-9,]+", row.cfg(cus)) for cus in (8, 64, 256, 304)), row.id
    for opts, fn, args, dflt, forced in lc.PREDICATES:
        assert set(opts) <= names and fn in nat.SIGNATURES and len(args) == len(nat.SIGNATURES[fn]), (opts, fn)
    for table in (lc.AUTO, lc.REQUEST):
        ids = [r.id for r in table]
        assert len(ids) == len(set(ids))


def _rows_of(case_name):
    """M of a case from its name: the builders write M<rows>, <H>x<W>,nh.. with B1, or B<samples>,T<tokens>"""
    for pat in (r"\bM(\d+)", r"\b(\d+)x(\d+),nh", r"\bB(\d+),T(\d+)"):
        m = re.search(pat, case_name)
        if m:
            g = [int(v) for v in m.groups()]
            return g[0] if len(g) == 1 else g[0] * g[1]
    raise AssertionError(case_name)


def test_auto_rows_cover_both_panel_branches_and_a_ragged_panel():
    """Every n-split axis has rows whose panel count is a multiple of 8 (panel_split's XCD branch), rows where it is not, and a ragged last panel --
    with more than one split forced, which is where the branch matters."""
    for option in ("x3_splits", "astat_splits", "mx8_splits"):
        ms = {_rows_of(r.case.name) for r in lc.AUTO if r.opts.get(option, 1) > 1}
        panels = {-(-m // 128) for m in ms}
        assert any(p % 8 == 0 for p in panels) and any(p % 8 for p in panels), (option, sorted(ms))
        assert any(m % 128 for m in ms), (option, sorted(ms))
    ms = {_rows_of(r.case.name) for r in lc.AUTO if r.opts.get("x3_splits", 1) > 1}          # split3: a ragged last panel on both branches
    assert any(m % 128 and -(-m // 128) % 8 == 0 for m in ms) and any(m % 128 and -(-m // 128) % 8 for m in ms), sorted(ms)


def test_cfg_matcher_refuses_the_right_kernel_under_another_configuration():
    """A fake op on the CPU that "launches" gemm_x3_astat<e0> with 2 splits whatever was asked for: the guard protocol passes (the arithmetic is
    right), the served-by assertion of a row that forced 4 splits must not."""
    launched = []

    def op(x, out):
        launched.append("gemm_x3_astat<e0> M=5 N=7 K=8 cfg=splits2")
        return out.copy_(2 * x)

    def make(env):
        x = torch.randn(5, 7, generator=torch.Generator().manual_seed(1))
        return dict(ins={"x": x}, outs={"y": ((5, 7), torch.float32)}, call=lambda T: op(T["x"], T["y"]), ref=lambda R: 2 * R["x"], tol=1e-6)
    run_case(Case("fake", "double", "fake", make), "nan")
    assert launched
    lc.assert_served("fake", launched, "gemm_x3_astat<e0>", "splits2")
    lc.assert_served("fake", launched, "gemm_x3_astat<e0>", None)
    for kernel, cfg in (("gemm_x3_astat<e0>", "splits4"), ("gemm_x3_astat<e0>", "splits"), ("gemm_x3_astat<e0>", "splits22"), ("gemm_x3_astat<e0,h>", "splits2"),
                        ("gemm_x3_astat<e2>", "splits2")):
        with pytest.raises(AssertionError, match="tested nothing"):
            lc.assert_served("fake", launched, kernel, cfg)
    # a launch site that states no configuration cannot serve a row that expects one; fields behind cfg= do not leak into it
    with pytest.raises(AssertionError):
        lc.assert_served("fake", ["gemm_x3_astat<e0> M=5 N=7 K=8"], "gemm_x3_astat<e0>", "splits2")
    assert lc.cfg_of("gemm_bf16_tiled<a0,e1> M=300 N=256 K=256 cfg=bm256,lw0,deep0") == "bm256,lw0,deep0"
    assert lc.cfg_of("attn_global_bf16 cfg=qw4") == "qw4" and lc.cfg_of("attn_global_bf16") is None
    assert lc.served(["gemm_bf16_astat<e5> M=8, N=8, K=8 cfg=rows128,splits3"], "gemm_bf16_astat<e5>", "rows128,splits3")


def test_restated_split_rule():
    # kd_common.h: best_n_splits -- ties go to fewer splits; one round of the chip is filled before tiles are shared out
    assert lc.best_n_splits(8, 12, 512, 2) == 12 and lc.best_n_splits(512, 12, 512, 2) == 1 and lc.best_n_splits(9, 6, 256, 1) == 6
    assert lc.best_n_splits(300, 4, 256, 1) == 2          # rounds x (1 + tiles): 2 x 5, 3 x 3, 5 x 2
    assert lc.tiled_cfg(300, 256, 1536, 128, 1)(256) == "bm128,lw1,deep1" and lc.tiled_cfg(300, 256, 1536, 256, 1)(256) == "bm256,lw0,deep0"
    assert lc.tiled_cfg(300, 256, 256, 128, 1)(256) == "bm128,lw0,deep0"
    assert lc.tiled_cfg(65536, 256, 256)(256) == "bm256,lw0,deep0"


@pytest.mark.parametrize("entry", lc.PREDICATES, ids=lambda e: f"{e[1]}{e[2]}|" + ",".join(f"{k}={v}" for k, v in e[0].items()))
def test_predicate_switches(entry):
    """The switches and thresholds that act through a ``*_supported`` predicate, which the model's launch plan asks (kd_ffn_bf16 / kd_ffn_f32 themselves
    launch whatever they are handed): the answer by default and with the option set.  No launch -- the forwards are PLAN_ROWS of
    tests/test_launch_config_gpu.py; the options go back to their defaults."""
    opts, fn, args, dflt, forced = entry
    f = getattr(nat.lib(), fn)
    assert f(*args) == dflt
    try:
        for k, v in opts.items():
            nat.set_option(k, v)
        assert f(*args) == forced
    finally:
        for k in opts:
            nat.set_option(k, lc.RESET)
    assert f(*args) == dflt

"""The one-wave-per-SIMD split3 kernels at the shapes where their request / ring-slot arithmetic can go wrong (csrc/ffn_x3.hip width 256,
csrc/gemm_x3.hip K = 512), through the ordinary op entry points in mode split3.  Needs a real MI355X.

Width-256 feed-forward block, with and without the fused out projection: d_ff = 64 / 128 / 192 / 768 are 1, 2, 3 and 12 tiles -- fewer
tiles than the request distance (every request past the first tile is one past the end of the stream), both parities of the ring's
starting slot, and the model's own count.  K = 512 norm -> GEGLU / qkv projections: one n-tile per workgroup, and more n-tiles than
n-splits (option x3_splits; the qkv epilogue's N is a multiple of 384 = 3 n-tiles, so "one n-tile" is three n-splits there).
Row counts 1 / 127 / 128 / 129 / 384: a single row, a ragged and a full panel, a panel + 1 row, three panels; each with all rows under one
sample's scale vector and (from 127 rows on) with samples so short that a wave's 32 rows straddle several.

Yardstick: the `exact` (fp32 FMA-order) mode's result of the same computation -- for the projections the same op under KDIFF_GEMM=exact, for
the fused block, which only exists in the bf16 / split3 modes, the ops the exact mode runs for it (out projection with residual, norm ->
GEGLU, down projection with residual) -- at the split3 bound of tests/test_ops_gpu.py (test_fused_feed_forward_split3,
test_split3_projections_round3: 1e-4, max-norm relative); and two runs give the same bits.  The guard-band cases (tests/test_bounds_gpu.py's
builders) add the one-tile and the 127-row shapes to those that file already has for these kernels."""
import numpy as np
import pytest
import torch

from k_diffusion_amd import _native as nat
from oracle import hdit
from tests import test_bounds_gpu as tb
from tests.guard import run_case
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
RESET = -2 ** 31
# (rows, samples): one sample for all rows; 127 samples of 1 row, 8 of 16, 3 of 43, 8 of 48 rows -- no wave's 32 rows inside one sample
LAYOUTS = [(1, 1), (127, 1), (127, 127), (128, 1), (128, 8), (129, 1), (129, 3), (384, 1), (384, 8)]


@pytest.fixture(scope="module")
def ops(KD):
    return KD.ops


@pytest.fixture
def split3_x3(KD, monkeypatch):
    """split3 mode with gemm_x3.hip taking every row count (it is chosen from 512 rows on by default) and the few-rows kernels off, as
    in tests/test_ops_gpu.py; `splits(n)` forces the n-split count.  Everything back to the built-in defaults afterwards."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    for k, v in (("x3s_max_rows", 0), ("b16s_max_rows", 0), ("x3_min_rows", 1)):
        nat.set_option(k, v)
    try:
        yield lambda n: nat.set_option("x3_splits", n)
    finally:
        for k in ("x3s_max_rows", "b16s_max_rows", "x3_min_rows", "x3_splits"):
            nat.set_option(k, RESET)


def rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


_GPU = {}


def g(key, make):
    """a seeded operand on the device, made once and shared (never written: every op below gets an `out` of its own)"""
    if key not in _GPU:
        _GPU[key] = make().to(DEV).contiguous()
    return _GPU[key]


def profiled(fn):
    lib = nat.lib()
    lib.kd_prof_reset()
    lib.kd_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [n.replace(", ", ",") for n in tb._prof_names()]
    finally:
        lib.kd_prof_enable(0)
        lib.kd_prof_reset()
    return out, names


def exact_mode(monkeypatch, fn):
    with monkeypatch.context() as m:
        m.setenv("KDIFF_GEMM", "exact")
        out = fn()
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fused_out", [False, True], ids=["ff", "out+ff"])
@pytest.mark.parametrize("dff", [64, 128, 192, 768])
@pytest.mark.parametrize("M,B", LAYOUTS)
def test_ffn_width_256(ops, split3_x3, monkeypatch, M, B, dff, fused_out):
    K, T = 256, M // B
    x = g(("x", M), lambda: rn(M, K, seed=41)).view(B, T, K)
    att = g(("att", M), lambda: rn(M, K, seed=42)).view(B, T, K)
    scale = g(("s", B), lambda: 1 + 0.2 * rn(B, K, seed=43))
    wo = g("wo", lambda: rn(K, K, seed=44, scale=K ** -0.5))
    wu = g(("wu", dff), lambda: rn(2 * dff, K, seed=45, scale=K ** -0.5))
    wd = g(("wd", dff), lambda: rn(K, dff, seed=46, scale=dff ** -0.5))
    kw = dict(attn=att, w_out=wo) if fused_out else {}

    y, names = profiled(lambda: ops.ffn(x, scale, wu, wd, rows_per_sample=T, **kw))
    want = f"ffn_x3{'+out' if fused_out else ''} M={M} K=256 d_ff={dff}"
    assert any(n.startswith(want) for n in names), (want, names)
    again = ops.ffn(x, scale, wu, wd, rows_per_sample=T, **kw)

    def exact():
        x1 = ops.linear(att, wo, residual=x) if fused_out else x
        hid = ops.norm_linear(x1, scale, wu, rows_per_sample=T, epi=nat.EPI_GEGLU)
        return ops.linear(hid, wd, residual=x1)
    ref = exact_mode(monkeypatch, exact)
    err = relerr(y, ref)
    print(f"ffn M={M} B={B} d_ff={dff} fused_out={fused_out}: relerr vs exact {err:.3e}")
    assert err < TOL
    assert torch.equal(y, again)


def _grid(T):
    """a token grid of T tokens (the qkv epilogue takes its RoPE angles from the tokens' positions)"""
    h = max(d for d in range(1, int(T ** 0.5) + 1) if T % d == 0)
    return h, T // h


@pytest.mark.parametrize("kind,N,splits", [("geglu", 64, 0), ("geglu", 320, 2), ("qkv", 384, 3), ("qkv", 384, 2)])
@pytest.mark.parametrize("M,B", LAYOUTS)
def test_projections_k512(ops, split3_x3, monkeypatch, M, B, kind, N, splits):
    K, T = 512, M // B
    x = g(("x512", M), lambda: rn(M, K, seed=51)).view(B, T, K)
    scale = g(("s512", B), lambda: 1 + 0.2 * rn(B, K, seed=52))
    if kind == "geglu":
        w = g(("wg512", N), lambda: rn(2 * N, K, seed=53, scale=K ** -0.5))

        def call():
            return ops.norm_linear(x, scale, w, rows_per_sample=T, epi=nat.EPI_GEGLU)
        want = f"gemm_x3_astat<e{nat.EPI_GEGLU}> M={M} N={N} K=512"
    else:
        nh, (H, W) = N // 192, _grid(T)
        w = g(("wq512", N), lambda: rn(N, K, seed=54, scale=K ** -0.5))
        theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).reshape(T, nh, 16)
        qk = (g(("qs", nh), lambda: torch.linspace(5.0, 12.0, nh)), g(("cos", T, nh), lambda: torch.cos(theta)), g(("sin", T, nh), lambda: torch.sin(theta)), nh,
              g(("pos", T), lambda: hdit.axial_pos(H, W).reshape(T, 2)), g(("fr", nh), lambda: hdit.rope_freqs(nh) / (2 * np.pi)))

        def call():
            return ops.norm_linear(x, scale, w, rows_per_sample=T, epi=nat.EPI_QKV, qk=qk)
        want = f"gemm_x3_astat<e{nat.EPI_QKV}> M={M} N={N} K=512"
    split3_x3(splits)
    y, names = profiled(call)
    assert any(n.startswith(want) for n in names), (want, names)
    if splits:
        assert any(f"cfg=splits{splits}" in n for n in names), names
    again = call()
    split3_x3(RESET)
    ref = exact_mode(monkeypatch, call)
    err = relerr(y, ref)
    print(f"{kind} M={M} B={B} N={N} splits={splits}: relerr vs exact {err:.3e}")
    assert err < TOL
    assert torch.equal(y, again)


# ---- guard bands: nothing outside the weight images (or any other tensor) is read, nothing outside the output written -------------------
GUARD = []
with tb.collect_into(GUARD):
    for _lead, _dff in [((1, 127), 64), ((1, 127), 768), ((2, 192), 64), ((1, 1), 64)]:      # one tile; 127 rows; one tile over three panels; one row
        _tag = "x".join(map(str, _lead))
        tb._ffn(f"ffn[split3,{_tag},K256,dff{_dff}]", _lead, 256, _dff, False, kernel="ffn_x3")
        tb._ffn(f"ffn[split3,attn,{_tag},K256,dff{_dff}]", _lead, 256, _dff, False, fused_out=True, kernel="ffn_x3+out")
    tb._lin("norm_geglu_ps", 127, 64, 512, "split3", B=1, kernel="gemm_x3_astat", src="gemm_x3.hip")
    tb._lin("norm_geglu_ps", 127, 320, 512, "split3", B=127, kernel="gemm_x3_astat", src="gemm_x3.hip")
    tb._qkv("norm_linear[qkv,split3,127x1,nh2,B1,K512]", 127, 1, 2, 1, 512, "split3", kernel="gemm_x3_astat<e5>", src="gemm_x3.hip")


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in GUARD])
def test_guard_bands(ops, split3_x3, c):
    (res, names) = profiled(lambda: run_case(c, "nan", env=ops, device=DEV))
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}; launches {sorted(set(names))}")
    assert any(n.startswith(c.kernel) for n in names), f"{c.name}: expected a launch of {c.kernel}*, the profile has {sorted(set(names))}"

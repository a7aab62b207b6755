"""Guard-band tests (tests/guard.py): no kernel reads or writes outside its tensors, and every output element is written.

One parametrized test over a case table; one case is one launch path of one op at one shape.  Every case runs the op on guarded views
(inputs with NaN-filled and with FLT_MAX-filled guards, outputs with 0xA5 guards around a NaN payload) and checks: the result against a
plain fp64 reference (torch on the CPU, or the oracle's functions) at the tolerance the op's existing test uses -- cited per builder --
the same bits as the ordinary call, the same bits under both fills, guards and inputs untouched, nothing left unwritten.  Ops without an
``out=`` argument get guarded inputs only (the result checks still see a NaN the kernel left or let in).  Needs a real MI355X.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.autograd.functional import jvp as fd_jvp

from k_diffusion_amd import _native as nat
from oracle import brownian as obrown
from oracle import hdit, solvers
from tests.guard import Case, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64, U8, I64 = torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int64


@pytest.fixture(scope="module")
def ops(KD):
    return KD.ops


def _prof_names():
    lib, out = nat.lib(), []
    name, ms, fl, by = C.create_string_buffer(128), C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.kd_prof_count()):
        nat.check(lib.kd_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)), "kd_prof_get")
        out.append(name.value.decode())
    return out


def rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ru(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def rt(t):
    """what a bf16 kernel sees of an fp32 value (dtype kept)"""
    return t.to(BF).to(t.dtype)


def rms(x, scale, eps=1e-6):
    return x * torch.rsqrt(x.square().mean(-1, keepdim=True) + eps) * scale


def geglu(h):
    d = h.shape[-1] // 2
    return h[..., :d] * F.gelu(h[..., d:])


def tables(h, w, nh):
    theta = hdit.rope_theta(hdit.axial_pos(h, w), hdit.rope_freqs(nh)).reshape(h * w, nh, 16)
    return torch.cos(theta), torch.sin(theta)


def pack(q, k, v):
    return torch.stack([q, k, v], dim=3).reshape(*q.shape[:3], -1).contiguous()


def split_stored(x):
    """fp32 [..., 64] -> the qkv_packed storage (tests/test_ops_gpu.py: _split_stored)"""
    hi = x.to(BF)
    lo = (x - hi.float()).to(BF)
    sh = x.shape[:-1]
    return torch.cat([hi.view(*sh, 16, 4), lo.view(*sh, 16, 4)], dim=-1).contiguous().view(F32).view(*sh, 64)


def unsplit(packed):
    """the values a split-stored tensor holds: hi + lo of every (hi x 4, lo x 4) bf16 group"""
    pw = packed.contiguous().view(torch.int32).view(-1, 4)
    hi = torch.stack([(pw[:, 0] << 16), (pw[:, 0] & -65536), (pw[:, 1] << 16), (pw[:, 1] & -65536)], dim=1).view(F32)
    lo = torch.stack([(pw[:, 2] << 16), (pw[:, 2] & -65536), (pw[:, 3] << 16), (pw[:, 3] & -65536)], dim=1).view(F32)
    return (hi + lo).view(packed.shape)


def np_mask(key, site, p, n):
    """The dropout mask contract (include/kdiff_hip.h) restated: element e keeps iff word e & 3 of philox4x32_10(key, e >> 2, site) >=
    floor(p 2^32); kept elements are multiplied by (float)(1 / (1 - p)), dropped ones by 0.  The float32 multipliers."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = obrown.philox4x32_10(key & (2 ** 64 - 1), q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), site & 0xFFFFFFFF, site >> 32)
    w = np.stack(np.broadcast_arrays(*words), axis=1).reshape(-1)[:n]
    keep = w >= np.uint32(int(np.floor(p * 2.0 ** 32)))
    return np.where(keep, np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)


CASES = []


@contextlib.contextmanager
def collect_into(table):
    """Inside the block the builders below append their cases to ``table`` instead of this module's CASES (tests/test_launch_config_gpu.py
    builds its rows with them); what this module collects and asserts does not change."""
    global CASES
    saved, CASES = CASES, table
    try:
        yield table
    finally:
        CASES = saved


def case(name, op, src, mode=None, few_rows=False, kernel=None):
    def deco(make):
        CASES.append(Case(name, op, src, make, mode=mode, few_rows=few_rows, kernel=kernel))
        return make
    return deco


# ---- GEMM-class ops -------------------------------------------------------------------------------------------------------------------
# tolerances: test_gemm_plain_and_residual / test_norm_linear_and_geglu (gtol: 2e-5 exact, 1e-4 split3), test_skinny_gemm_rows_per_sample
# (2e-5), test_bf16_gemm_plain_and_residual (8e-3), test_bf16_norm_linear_and_geglu (1.2e-2 store, 1.5e-2 GEGLU), test_bf16_qkv_epilogue (1.2e-2)
GTOL = {"exact": 2e-5, "split3": 1e-4}


def _route(kind, M, N, K, mode, bf, few_rows, rps):
    """The launch-profile name (up to the shape) of the kernel that serves a plain-A projection, restated from the dispatch of kd_gemm_f32
    (gemm.hip) and kd_gemm_bf16 (gemm_bf16.hip) for the kinds of ``_lin``; the a-stationary / residual split3 kernels are named by the case."""
    norm = int("norm" in kind)
    epi = nat.EPI_GEGLU if "geglu" in kind else (nat.EPI_RESIDUAL if kind.startswith("res") else nat.EPI_STORE)
    if not bf:
        if few_rows:
            return "gemm_x3s<"
        if M <= 128 and not kind.endswith("_ps"):                    # one gain for all rows, at most 128 rows: the fp32 skinny kernel in both modes
            return f"gemm_skinny<n{norm},e{epi}>"
        return f"gemm_{'bf16x3' if mode == 'split3' else 'f32'}<a0,n{norm},e{epi}>"
    if few_rows:
        return "gemm_bf16_few_rows<"
    add = kind == "add"
    wstat = (K in (128, 256, 384, 512) and N % 32 == 0 and M >= 2048 and not (epi == nat.EPI_RESIDUAL and norm)
             and (epi in (nat.EPI_RESIDUAL, nat.EPI_STORE) or norm) and not add and (not norm or rps % 32 == 0))
    if wstat and (K == 128 or (K == 384 and N <= 128)):
        return f"gemm_bf16_wstat<e{epi},n{norm}>"
    if norm and K in (256, 512) and epi != nat.EPI_RESIDUAL and not add and M >= 512:
        return f"gemm_bf16_astat<e{epi}>"
    if not norm and K % 64 == 0 and N % 32 == 0 and epi != nat.EPI_GEGLU and not add:
        return f"gemm_bf16_tiled<a0,e{epi}>"
    if wstat:
        return f"gemm_bf16_wstat<e{epi},n{norm}>"
    return f"gemm_bf16_generic<a0,e{epi}>"


def _lin(kind, M, N, K, mode, bf=False, tol=None, B=None, few_rows=False, kernel=None, src=None, tag=""):
    """kind: plain / res / res_inplace / add / geglu / norm (shared gain) / norm_ps (per-sample scales, B samples) / norm_geglu(_ps)"""
    tol = tol if tol is not None else (GTOL[mode] if not bf else {"geglu": 1.5e-2}.get(kind.replace("norm_", "").replace("_ps", ""), 1.2e-2 if "norm" in kind else 8e-3))
    op = {"plain": "linear", "res": "linear", "res_inplace": "linear", "add": "linear", "geglu": "linear_geglu"}.get(kind, "norm_linear")
    src = src or ("gemm_bf16.hip" if bf else "gemm.hip")
    name = f"{op}[{kind}{tag},{'bf16' if bf else mode},M{M},N{N},K{K}{',few' if few_rows else ''}]"
    kernel = kernel or _route(kind, M, N, K, mode, bf, few_rows, M // B if kind.endswith("_ps") else M)
    if kernel.startswith("gemm_skinny"):
        src = "gemm_skinny.hip"

    def make(ops):
        dt = BF if bf else F32
        wr = rt if bf else (lambda t: t)
        x = rn(M, K, seed=1).to(dt)
        two = 2 if "geglu" in kind else 1
        ins = {"x": x, "w": rn(two * N, K, seed=2) / K ** 0.5}
        outs = {"y": ((M, N), dt)}
        inplace = ()
        if kind in ("res", "res_inplace"):
            ins["r"] = rn(M, N, seed=3).to(dt)
        if kind == "res_inplace":
            outs, inplace = {}, ("r",)
        if "norm" in kind:
            ins["s"] = 1 + 0.2 * (rn(B, K, seed=5) if kind.endswith("_ps") else rn(K, seed=5))
        rps = M // B if kind.endswith("_ps") else M

        def call(T):
            if kind == "plain":
                return ops.linear(T["x"], T["w"], out=T["y"])
            if kind == "res":
                return ops.linear(T["x"], T["w"], residual=T["r"], out=T["y"])
            if kind == "res_inplace":
                return ops.linear(T["x"], T["w"], residual=T["r"], out=T["r"])
            if kind == "add":
                return ops.linear(T["x"], T["w"], out_add=1.0, out=T["y"])
            if kind == "geglu":
                return ops.linear_geglu(T["x"], T["w"], out=T["y"])
            return ops.norm_linear(T["x"], T["s"], T["w"], rows_per_sample=rps, epi=nat.EPI_GEGLU if "geglu" in kind else nat.EPI_STORE, out=T["y"])

        def ref(R):
            a = R["x"]
            if "norm" in kind:
                a = rms(a.view(-1, rps, K), R["s"].view(-1, 1, K)).view(M, K)
            y = a @ wr(R["w"]).T
            if "geglu" in kind:
                y = geglu(y)
            return y + (R["r"] if "r" in R else 0) + (1.0 if kind == "add" else 0.0)
        return dict(ins=ins, outs=outs, call=call, ref=ref, tol=tol, inplace=inplace)
    CASES.append(Case(name, op, src, make, mode=None if bf else mode, few_rows=few_rows, kernel=kernel))


for _M, _N, _K in [(5, 28, 12), (131, 200, 96), (257, 129, 48), (1000, 48, 128)]:
    for _kind in ("plain", "res", "add", "geglu", "norm", "norm_geglu"):
        _lin(_kind, _M, _N, _K, "exact")
        _lin(_kind, _M, _N, _K, "split3")
for _M, _N, _K in [(1, 256, 256), (7, 12, 12), (65, 8, 256)]:
    for _kind in ("plain", "res", "add", "geglu", "norm", "norm_geglu"):
        _lin(_kind, _M, _N, _K, "exact", tol=2e-5, kernel="gemm_skinny", src="gemm_skinny.hip")
    for _mode in ("exact", "split3"):         # per-sample scale vectors with rows_per_sample = 1: the tile kernels keep serving them
        _lin("norm_ps", _M, _N, _K, _mode, B=_M, tag=",rps1")
# the a-stationary wide projections and the residual projection (test_wide_projections_a_stationary, test_residual_in_place_multi_tile: 1e-4)
_lin("norm_geglu", 1000, 768, 128, "split3", kernel="gemm_x3_astat", src="gemm_x3.hip")
_lin("norm", 520, 256, 128, "split3", kernel="gemm_x3_astat", src="gemm_x3.hip")
_lin("norm_ps", 1000, 256, 128, "split3", B=4, kernel="gemm_x3_astat", src="gemm_x3.hip")
for _M in (1000, 520):
    _lin("res", _M, 256, 256, "split3", kernel="gemm_x3r", src="gemm_x3r.hip")
    _lin("res_inplace", _M, 256, 256, "split3", kernel="gemm_x3r", src="gemm_x3r.hip")
# the few-rows kernels at their defaults (test_split3_few_rows_latency_kernel: 1e-4; test_bf16_few_rows...: the bf16 bounds)
for _H, _W, _B, _K in [(6, 6, 4, 64), (9, 12, 3, 128), (7, 7, 4, 256)]:
    for _kind in ("norm_ps", "norm_geglu_ps", "res", "norm"):
        _lin(_kind, _H * _W * _B, 256 if _kind != "norm_geglu_ps" else 3 * _K, _K if _kind != "res" else 3 * _K, "split3", B=_B, few_rows=True, kernel="gemm_x3s", src="gemm_x3s.hip")
for _kind in ("norm_ps", "norm_geglu_ps", "res"):
    _lin(_kind, 7 * 7 * 4, 256, 256, None, bf=True, B=4, few_rows=True, kernel="gemm_bf16_few_rows", src="gemm_b16s.hip")
# bf16
for _M, _N, _K in [(70, 32, 12), (300, 160, 64), (1000, 96, 192)]:
    for _kind in ("plain", "res", "res_inplace"):
        _lin(_kind, _M, _N, _K, None, bf=True)
for _kind in ("norm_ps", "norm_geglu_ps", "norm"):
    _lin(_kind, 520, 256, 256, None, bf=True, B=2, kernel="gemm_bf16_astat")
for _kind in ("plain", "res", "res_inplace", "norm_ps", "norm_geglu_ps"):
    _lin(_kind, 2080, 96, 128, None, bf=True, B=5, kernel="gemm_bf16_wstat")          # 5 samples of 416 = 13 x 32 rows; 16 row panels and a quarter
for _B, _T, _K, _dff in [(2, 50, 100, 96), (4, 49, 256, 768)]:
    _lin("norm_ps", _B * _T, _dff, _K, None, bf=True, B=_B)
    _lin("norm_geglu_ps", _B * _T, _dff, _K, None, bf=True, B=_B)


def _qkv(name, H, W, nh, B, K, mode, bf=False, packed=False, few_rows=False, kernel=None, src="gemm.hip", block=None):
    """EPI_QKV (test_qkv_epilogue_prepares_q_and_k: gtol; test_split3_projections_round3: 1e-4 and 2^-15 for the split-stored form;
    test_bf16_qkv_epilogue: 1.2e-2; test_attn_block_bf16_matches_two_launches: 2e-2; test_proj_block_bf16...: the projection's bound)"""
    op = "norm_linear" if block is None else block

    def make(ops):
        T_, d = H * W, nh * 64
        dt = BF if bf else F32
        ins = {"x": rn(B, T_, K, seed=8).to(dt), "s": 1 + 0.2 * rn(B, K, seed=9), "w": rn(3 * d, K, seed=10, scale=K ** -0.5),
               "sh": torch.linspace(5.0, 12.0, nh), "pos": hdit.axial_pos(H, W).reshape(T_, 2).contiguous(),
               "fr": (hdit.rope_freqs(nh) / (2 * np.pi)).contiguous()}
        if not bf:
            ins["cos"], ins["sin"] = tables(H, W, nh)
        out_shape = (B, T_, K) if block == "attn_block" else (B, T_, 3 * d)

        def call(T):
            qk = (T["sh"], T["pos"], T["fr"], nh) if bf else (T["sh"], T["cos"], T["sin"], nh, T["pos"], T["fr"])
            if block == "attn_block":
                return ops.attn_block(T["x"], T["s"], T["w"], rows_per_sample=T_, qk=qk, out=T["y"])
            if block == "proj_block":
                return ops.proj_block(T["x"], T["s"], T["w"], rows_per_sample=T_, epi=nat.EPI_QKV, qk=qk, out=T["y"])
            y = ops.norm_linear(T["x"], T["s"], T["w"], rows_per_sample=T_, epi=nat.EPI_QKV, qk=qk, qkv_packed=packed, out=T["y"])
            return unsplit(y) if packed else y

        def ref(R):
            w = rt(R["w"]) if bf else R["w"]
            r = (rms(R["x"], R["s"][:, None, :]) @ w.T).view(B, H, W, 3, nh, 64)
            theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
            q, k = hdit.cosine_sim_scale(r[..., 0, :, :], r[..., 1, :, :], R["sh"])
            q, k, v = hdit.apply_rope(q, theta), hdit.apply_rope(k, theta), r[..., 2, :, :]
            if block == "attn_block":
                return hdit.attn_global(q.reshape(B, 1, T_, nh, 64), k.reshape(B, 1, T_, nh, 64), v.reshape(B, 1, T_, nh, 64), 1.0).reshape(B, T_, K)
            return torch.stack([q, k, v], dim=3).reshape(B, T_, 3 * d)
        tol = (2e-2 if block == "attn_block" else 1.2e-2) if bf else GTOL[mode]
        return dict(ins=ins, outs={"y": (out_shape, dt)}, call=call, ref=ref, tol=tol)
    CASES.append(Case(name, op, src, make, mode=None if bf else mode, few_rows=few_rows, kernel=kernel))


_qkv("norm_linear[qkv,exact,16x8,nh2,B2]", 16, 8, 2, 2, 128, "exact", kernel="gemm_f32<a0,n1,e5>")
_qkv("norm_linear[qkv,split3,16x8,nh2,B2]", 16, 8, 2, 2, 128, "split3", kernel="gemm_bf16x3<a0,n1,e5>")
_qkv("norm_linear[qkv,split3,24x24,nh2,B1,K128]", 24, 24, 2, 1, 128, "split3", kernel="gemm_x3_astat<e5>", src="gemm_x3.hip")
_qkv("norm_linear[qkv_packed,split3,24x24,nh2,B1,K128]", 24, 24, 2, 1, 128, "split3", packed=True, kernel="gemm_x3_astat<e5>", src="gemm_x3.hip")
_qkv("norm_linear[qkv_packed,split3,12x20,nh4,B3,K256]", 12, 20, 4, 3, 256, "split3", packed=True, kernel="gemm_x3_astat<e5,h>", src="gemm_x3.hip")
_qkv("norm_linear[qkv,split3,few,7x7,nh4,B4,K256]", 7, 7, 4, 4, 256, "split3", few_rows=True, kernel="gemm_x3s", src="gemm_x3s.hip")
_qkv("norm_linear[qkv_packed,split3,few,9x12,nh2,B3,K128]", 9, 12, 2, 3, 128, "split3", packed=True, few_rows=True, kernel="gemm_x3s", src="gemm_x3s.hip")
_qkv("norm_linear[qkv,bf16,7x7,nh4,B3,K256]", 7, 7, 4, 3, 256, None, bf=True, kernel="gemm_bf16_generic<a0,e5>", src="gemm_bf16.hip")
_qkv("norm_linear[qkv,bf16,20x13,nh4,B2,K256]", 20, 13, 4, 2, 256, None, bf=True, kernel="gemm_bf16_astat<e5>", src="gemm_bf16.hip")
_qkv("norm_linear[qkv,bf16,few,7x7,nh4,B4,K256]", 7, 7, 4, 4, 256, None, bf=True, few_rows=True, kernel="gemm_bf16_few_rows", src="gemm_b16s.hip")
_qkv("attn_block[16x16,nh4,B3,K256]", 16, 16, 4, 3, 256, None, bf=True, block="attn_block", kernel="attn_block_bf16", src="block_bf16.hip")
_qkv("proj_block[qkv,16x16,nh4,B3,K256]", 16, 16, 4, 3, 256, None, bf=True, block="proj_block", kernel="proj_block_bf16", src="block_bf16.hip")


@case("proj_block[geglu,B3,T256,K256,dff384]", "proj_block", "block_bf16.hip", kernel="proj_block_bf16")
def _(ops):
    B, T_, K, d_ff = 3, 256, 256, 384
    ins = {"x": rn(B, T_, K, seed=8).to(BF), "s": 1 + 0.2 * rn(B, K, seed=9), "w": rn(2 * d_ff, K, seed=7, scale=K ** -0.5)}
    return dict(ins=ins, outs={"y": ((B, T_, d_ff), BF)}, call=lambda T: ops.proj_block(T["x"], T["s"], T["w"], rows_per_sample=T_, out=T["y"]),
                ref=lambda R: geglu(rms(R["x"], R["s"][:, None, :]) @ rt(R["w"]).T), tol=1.5e-2)       # test_proj_block_bf16_matches_the_projection_kernel


def _planes(name, M, N, K, epi, c_planes):
    """a_planes / c_planes (gemm_x3t.hip; test_split3_projections_round3: 1e-4, 2^-15 for norm_split's planes)"""
    @case(name, "gemm", "gemm_x3t.hip", mode="split3", kernel="gemm_x3_tiled")
    def _(ops):
        a = rn(M, K, seed=1)
        hi = a.to(BF)
        lo = (a - hi.float()).to(BF)
        two = 2 if epi == nat.EPI_GEGLU else 1
        ins = {"hi": hi, "lo": lo, "w": rn(two * N, K, seed=2, scale=K ** -0.5)}
        if epi == nat.EPI_RESIDUAL:
            ins["r"] = rn(M, N, seed=3)
        outs = {"ch": ((M, N), BF), "cl": ((M, N), BF)} if c_planes else {"y": ((M, N), F32)}

        def call(T):
            if c_planes:
                ops.gemm(None, T["w"], None, M=M, N=N, K=K, epi=epi, a_planes=(T["hi"], T["lo"]), c_planes=(T["ch"], T["cl"]))
                return T["ch"], T["cl"]
            return ops.gemm(None, T["w"], T["y"], M=M, N=N, K=K, epi=epi, residual=T.get("r"), a_planes=(T["hi"], T["lo"]))

        def ref(R):
            y = (R["hi"] + R["lo"]) @ R["w"].T
            y = geglu(y) if epi == nat.EPI_GEGLU else y + (R["r"] if "r" in R else 0)
            return (y, y) if c_planes else y

        if c_planes:
            def call_sum(T):
                h, l = call(T)
                return h.float() + l.float(), h, l
            return dict(ins=ins, outs=outs, call=call_sum, ref=lambda R: (ref(R)[0], None, None), tol=[1e-4, None, None])
        return dict(ins=ins, outs=outs, call=call, ref=ref, tol=1e-4)


_planes("gemm[a_planes,store,M600,N128,K384]", 600, 128, 384, nat.EPI_STORE, False)
_planes("gemm[a_planes,residual,M600,N128,K384]", 600, 128, 384, nat.EPI_RESIDUAL, False)
_planes("gemm[a_planes,c_planes,geglu,M600,N384,K128]", 600, 384, 128, nat.EPI_GEGLU, True)


@case("norm_split[B2,T300,K128]", "norm_split", "gemm_x3t.hip", mode="split3", kernel="norm_split_f32")
def _(ops):
    B, T_, K = 2, 300, 128
    ins = {"x": rn(B, T_, K, seed=8), "s": 1 + 0.2 * rn(B, K, seed=9)}

    def call(T):
        h, l = ops.norm_split(T["x"], T["s"], rows_per_sample=T_)
        return h, h.float() + l.float()
    return dict(ins=ins, call=call, ref=lambda R: (rms(R["x"], R["s"][:, None, :]),) * 2, tol=[2.0 ** -8, 2.0 ** -15])      # test_split3_projections_round3


# ---- mx8 (test_gemm_mx8_vs_the_restated_arithmetic: 6e-3 store, 8e-3 GEGLU / qkv; test_gemm_mx8_tiled_form: 6e-3) ------------------------

def _mx8(B, T_, K, d_ff, kind):
    @case(f"norm_linear[mx8,{kind},B{B},T{T_},K{K},dff{d_ff}]", "norm_linear", "gemm_mx8.hip", kernel="gemm_mx8_astat")
    def _(ops):
        N = 2 * K if kind == "store" else d_ff
        x = rn(B, T_, K, seed=8) * (1 + rn(B, T_, 1, seed=3).abs())
        x[0, 0, 32:64] = 0.0
        ins = {"x": x.to(BF), "s": 1 + 0.2 * rn(B, K, seed=9), "w": rn(2 * N if kind == "geglu" else N, K, seed=11, scale=K ** -0.5)}

        def call(T):
            return ops.norm_linear(T["x"], T["s"], T["w"], rows_per_sample=T_, epi=nat.EPI_GEGLU if kind == "geglu" else nat.EPI_STORE, mx8=True, out=T["y"])

        def ref(R):
            xr = R["x"].float()
            rs = torch.rsqrt(xr.square().mean(-1, keepdim=True) + 1e-6)
            uq = hdit.mx8_quantize_rows(xr * R["s"].float()[:, None, :])
            h = (uq.double() @ hdit.mx8_quantize_weight(R["w"].float()).double().T) * rs.double()
            return geglu(h) if kind == "geglu" else h
        return dict(ins=ins, outs={"y": ((B, T_, N), BF)}, call=call, ref=ref, tol=8e-3 if kind == "geglu" else 6e-3)


def _mx8_ins(B, T_, K):
    x = rn(B, T_, K, seed=8) * (1 + rn(B, T_, 1, seed=3).abs())
    x[0, 0, 32:64] = 0.0
    return {"x": x.to(BF), "s": 1 + 0.2 * rn(B, K, seed=9)}


def _mx8_proj(R, w):
    xr = R["x"].float()
    rs = torch.rsqrt(xr.square().mean(-1, keepdim=True) + 1e-6)
    uq = hdit.mx8_quantize_rows(xr * R["s"].float()[:, None, :])
    return (uq.double() @ hdit.mx8_quantize_weight(w.float()).double().T) * rs.double()


def _mx8_qkv(B, T_, K, d_ff):
    @case(f"norm_linear[mx8,qkv,B{B},T{T_},K{K}]", "norm_linear", "gemm_mx8.hip", kernel="gemm_mx8_astat<e5>")
    def _(ops):
        nh = K // 64
        H, W = (T_ // 16, 16) if T_ % 16 == 0 else (T_, 1)
        ins = dict(_mx8_ins(B, T_, K), w=rn(3 * K, K, seed=10, scale=K ** -0.5), sh=torch.linspace(5.0, 12.0, nh),
                   pos=hdit.axial_pos(H, W).reshape(T_, 2).contiguous(), fr=(hdit.rope_freqs(nh) / (2 * np.pi)).contiguous())

        def call(T):
            y = ops.norm_linear(T["x"], T["s"], T["w"], rows_per_sample=T_, epi=nat.EPI_QKV, qk=(T["sh"], T["pos"], T["fr"], nh), mx8=True, out=T["y"])
            parts = y.view(B, H, W, 3, nh, 64)
            return parts[..., 0, :, :], parts[..., 1, :, :], parts[..., 2, :, :]

        def ref(R):
            r = _mx8_proj(R, R["w"]).view(B, H, W, 3, nh, 64)
            theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
            q, k = hdit.cosine_sim_scale(r[..., 0, :, :], r[..., 1, :, :], R["sh"])
            return hdit.apply_rope(q, theta), hdit.apply_rope(k, theta), r[..., 2, :, :]
        return dict(ins=ins, outs={"y": ((B, T_, 3 * K), BF)}, call=call, ref=ref, tol=8e-3)


def _mx8_c8(B, T_, K, d_ff):
    @case(f"norm_linear[mx8,geglu,c_fp8,B{B},T{T_},K{K},dff{d_ff}]", "norm_linear", "gemm_mx8.hip", kernel="gemm_mx8_astat<e2,c8>")
    def _(ops):
        ins = dict(_mx8_ins(B, T_, K), w=rn(2 * d_ff, K, seed=7, scale=K ** -0.5))

        def call(T):
            h8, hs = ops.norm_linear(T["x"], T["s"], T["w"], rows_per_sample=T_, epi=nat.EPI_GEGLU, mx8=True, c_fp8=True)
            dec = h8.cpu().view(torch.float8_e4m3fn).float().view(B, T_, d_ff // 32, 32) * torch.ldexp(torch.ones(()), hs.cpu().to(torch.int32) - 127)[..., None]
            return dec.view(B, T_, d_ff), dec.view(B, T_, d_ff).clone(), h8, hs

        def ref(R):
            h = geglu(_mx8_proj(R, R["w"])).float()
            return hdit.mx8_quantize_rows(h), h, None, None
        # the op allocates its two planes: guarded inputs only.  7e-2 twice, as in the existing test: the decoded planes against the restated quantiser on the
        # restated hidden, and against that hidden itself
        return dict(ins=ins, call=call, ref=ref, tol=[7e-2, 7e-2, None, None])


for _shape in [(2, 100, 512, 192), (1, 333, 256, 768)]:
    _mx8_qkv(*_shape)
    _mx8_c8(*_shape)
for _shape in [(2, 100, 512, 192), (1, 333, 256, 768)]:
    _mx8(*_shape, "store")
    _mx8(*_shape, "geglu")


def _mx8_tiled(res):
    @case(f"linear_mx8[M300,K512,N512{',res' if res else ''}]", "linear_mx8", "gemm_mx8.hip", kernel="gemm_mx8_tiled")
    def _(ops):
        M, K, N = 300, 512, 512
        u = rn(M, K, seed=4) * torch.logspace(-2, 2, K // 32).repeat_interleave(32)[None, :]
        u[5, 64:96] = 0.0
        blocks = u.view(M, K // 32, 32)
        s = hdit.mx8_scale(blocks.abs().amax(-1, keepdim=True))
        q8 = (blocks / s).to(torch.float8_e4m3fn)
        dec = (q8.float() * s).reshape(M, K).double()
        ins = {"a8": q8.view(U8).reshape(M, K).contiguous(), "sb": (torch.log2(s).round().to(torch.int32) + 127).to(U8).reshape(M, K // 32).contiguous(),
               "w": rn(N, K, seed=6, scale=K ** -0.5)}
        if res:
            ins["r"] = rn(M, N, seed=2).to(BF)
        return dict(ins=ins, outs={"y": ((M, N), BF)}, call=lambda T: ops.linear_mx8(T["a8"], T["sb"], T["w"], residual=T.get("r"), out=T["y"]),
                    ref=lambda R: dec @ hdit.mx8_quantize_weight(R["w"].float()).double().T + (R["r"] if res else 0), tol=6e-3)


_mx8_tiled(False)
_mx8_tiled(True)


# ---- fused feed-forward blocks (test_bf16_fused_ffn / _width_256: 8e-3; tests/test_attn_ffn_fused_gpu.py and the split3 ffn tests: 1e-4) ---

def _ffn(name, lead, K, d_ff, bf, fused_out=False, inplace=False, src=None, kernel=None):
    @case(name, "ffn", src or ("ffn_bf16.hip" if bf else "ffn_x3.hip"), mode=None if bf else "split3", kernel=kernel)
    def _(ops):
        dt = BF if bf else F32
        wr = rt if bf else (lambda t: t)
        B = lead[0]
        rows = int(np.prod(lead[1:]))
        ins = {"x": rn(*lead, K, seed=14).to(dt), "s": 1 + 0.2 * rn(B, K, seed=15), "wu": rn(2 * d_ff, K, seed=16, scale=K ** -0.5),
               "wd": rn(K, d_ff, seed=17, scale=d_ff ** -0.5)}
        if fused_out:
            ins["attn"], ins["wo"] = rn(*lead, K, seed=18).to(dt), rn(K, K, seed=19, scale=K ** -0.5)

        def call(T):
            return ops.ffn(T["x"], T["s"], T["wu"], T["wd"], rows_per_sample=rows, out=T["x"] if inplace else T["y"], attn=T.get("attn"), w_out=T.get("wo"))

        def ref(R):
            x = R["x"].view(B, rows, K)
            if fused_out:
                x = x + R["attn"].view(B, rows, K) @ wr(R["wo"]).T
            return (x + geglu(rms(x, R["s"][:, None, :]) @ wr(R["wu"]).T) @ wr(R["wd"]).T).view(*lead, K)
        return dict(ins=ins, outs={} if inplace else {"y": ((*lead, K), dt)}, call=call, ref=ref, tol=8e-3 if bf else 1e-4, inplace=("x",) if inplace else ())


for _B, _T, _dff in [(2, 300, 128), (1, 130, 64)]:
    _ffn(f"ffn[bf16,B{_B},T{_T},K128,dff{_dff}]", (_B, _T), 128, _dff, True, kernel="ffn_bf16")
    _ffn(f"ffn[bf16,inplace,B{_B},T{_T},K128,dff{_dff}]", (_B, _T), 128, _dff, True, inplace=True, kernel="ffn_bf16")
    _ffn(f"ffn[bf16,attn,B{_B},T{_T},K128,dff{_dff}]", (_B, _T), 128, _dff, True, fused_out=True, kernel="ffn_bf16+out")
_ffn("ffn[bf16,B2,T77,K256,dff192]", (2, 77), 256, 192, True, kernel="ffn_bf16")
_ffn("ffn[bf16,inplace,B2,T77,K256,dff192]", (2, 77), 256, 192, True, inplace=True, kernel="ffn_bf16")
for _K, _dff in [(128, 192), (256, 448)]:
    _ffn(f"ffn[split3,30x30,B3,K{_K},dff{_dff}]", (3, 30, 30), _K, _dff, False, kernel="ffn_x3")
    _ffn(f"ffn[split3,inplace,30x30,B3,K{_K},dff{_dff}]", (3, 30, 30), _K, _dff, False, inplace=True, kernel="ffn_x3")
    _ffn(f"ffn[split3,attn,30x30,B3,K{_K},dff{_dff}]", (3, 30, 30), _K, _dff, False, fused_out=True, kernel="ffn_x3+out")
    _ffn(f"ffn[split3,attn,inplace,30x30,B3,K{_K},dff{_dff}]", (3, 30, 30), _K, _dff, False, fused_out=True, inplace=True, kernel="ffn_x3+out")


def _attn_ffn(B, H, W, nh, ks, K, d_ff, inplace):
    @case(f"attn_ffn[{H}x{W},B{B},nh{nh},k{ks},K{K},dff{d_ff}{',inplace' if inplace else ''}]", "attn_ffn", "attn_ffn_x3.hip", mode="split3", kernel="attn_ffn_x3")
    def _(ops):
        assert ops.attn_ffn_supported(B, H, W, nh, ks, K, d_ff)
        q, k, v = (rn(B, H, W, nh, 64, seed=s, scale=sc) for s, sc in ((1, 0.5), (2, 0.5), (3, 1.0)))
        ins = {"qkv": pack(split_stored(q), split_stored(k), split_stored(v)), "x": rn(B, H, W, K, seed=14), "s": 1 + 0.2 * rn(B, K, seed=15),
               "wu": rn(2 * d_ff, K, seed=16, scale=K ** -0.5), "wd": rn(K, d_ff, seed=17, scale=d_ff ** -0.5), "wo": rn(K, K, seed=19, scale=K ** -0.5)}

        def ref(R):
            a = hdit.na2d(q.double(), k.double(), v.double(), ks, 1.0).reshape(B, H * W, K)
            x = R["x"].view(B, H * W, K) + a @ R["wo"].T
            return (x + geglu(rms(x, R["s"][:, None, :]) @ R["wu"].T) @ R["wd"].T).view(B, H, W, K)
        return dict(ins=ins, outs={} if inplace else {"y": ((B, H, W, K), F32)}, inplace=("x",) if inplace else (),
                    call=lambda T: ops.attn_ffn(T["qkv"], nh, ks, T["x"], T["s"], T["wu"], T["wd"], T["wo"], out=T["x"] if inplace else T["y"]),
                    ref=ref, tol=1e-4)          # tests/test_attn_ffn_fused_gpu.py


_attn_ffn(2, 32, 32, 2, 7, 128, 384, False)          # the smallest the predicate takes: 2048 rows, a token grid of 8 x 16 tiles
_attn_ffn(2, 32, 32, 2, 7, 128, 384, True)
_attn_ffn(3, 24, 32, 2, 7, 128, 192, False)          # 18 row panels over three samples, a non-square grid


# ---- patch / merge / split (test_token_merge_split, test_patch_in_out: gtol; test_token_split_multi_tile, test_split3_patch_out_round3: 1e-4;
# the bf16 forms: 1.2e-2, the projection bound of the bf16 mode) ------------------------------------------------------------------------------

def _merge_split(B, h, w, K, Cc, mode, bf=False):
    dt = BF if bf else F32
    wr = rt if bf else (lambda t: t)
    tol = 1.2e-2 if bf else GTOL[mode]
    x3r = mode == "split3" and not bf            # (the split runs on gemm_x3r.hip from K = 256, C = 128 on; the merge at both shapes)
    src = "gemm_bf16.hip" if bf else ("gemm_x3r.hip" if x3r else "gemm.hip")
    tag = f"{'bf16' if bf else mode},B{B},{h}x{w},K{K},C{Cc}"

    @case(f"token_merge[{tag}]", "token_merge", src, mode=None if bf else mode, kernel="gemm_bf16_tiled<a1" if bf else ("gemm_x3r<a1" if x3r else "gemm_f32<a1"))
    def _(ops):
        ins = {"x": rn(B, 2 * h, 2 * w, Cc, seed=1).to(dt), "w": rn(K, 4 * Cc, seed=2, scale=(4 * Cc) ** -0.5)}
        return dict(ins=ins, outs={"y": ((B, h, w, K), dt)}, call=lambda T: ops.token_merge(T["x"], T["w"], out=T["y"]),
                    ref=lambda R: hdit.token_merge(R["x"], wr(R["w"]), 2, 2), tol=tol)

    for inplace in (False, True):
        @case(f"token_split_lerp[{tag}{',inplace' if inplace else ''}]", "token_split_lerp", src if not x3r or K >= 256 else "gemm.hip", mode=None if bf else mode,
              kernel="gemm_x3r<a0,e3>" if x3r and K >= 256 else ("gemm_bf16_tiled<a0,e3>" if bf else f"gemm_{'bf16x3' if mode == 'split3' else 'f32'}<a0,n0,e3>"))
        def _(ops, inplace=inplace):
            ins = {"x": rn(B, h, w, K, seed=1).to(dt), "w": rn(4 * Cc, K, seed=2) / K ** 0.5, "skip": rn(B, 2 * h, 2 * w, Cc, seed=3).to(dt), "fac": torch.tensor([0.3])}
            return dict(ins=ins, outs={} if inplace else {"y": ((B, 2 * h, 2 * w, Cc), dt)}, inplace=("skip",) if inplace else (),
                        call=lambda T: ops.token_split_lerp(T["x"], T["w"], T["skip"], T["fac"], out=T["skip"] if inplace else T["y"]),
                        ref=lambda R: torch.lerp(R["skip"], hdit.token_split(R["x"], wr(R["w"]), 2, 2), R["fac"]), tol=tol)


for _shape in [(3, 16, 12, 128, 64), (3, 20, 12, 256, 128)]:
    _merge_split(*_shape, "exact")
    _merge_split(*_shape, "split3")
    _merge_split(*_shape, None, bf=True)


def _patch(Cc, H, W, p, d, mode, bf=False, sigma=False, B=3):
    dt = BF if bf else F32
    wr = rt if bf else (lambda t: t)
    tol = 1.2e-2 if bf else GTOL[mode]
    M, feat = B * (H // p) * (W // p), Cc * p * p
    # restated from the dispatch: gemm_x3.hip's a-stationary unpatch kernel (split3: K = 128, 4 x 4 patches, at most 4 channels, from x3_min_rows =
    # 512 rows on) and patch_bf16.hip's gemm_patch_try (4-wide patches, at most 64 patch features; unpatch: features a multiple of 8, K in {128, 256};
    # patch-in: N a multiple of 128, at most 512); everything else is the generic kernel of the mode
    x3_out = mode == "split3" and d == 128 and p == 4 and feat <= 64 and M >= 512
    bf_out = bf and p == 4 and feat <= 64 and feat % 8 == 0 and d in (128, 256)
    bf_in = bf and p == 4 and feat <= 64 and d % 128 == 0 and d <= 512
    gen = "gemm_bf16_generic<a{a},e{e}>" if bf else ("gemm_bf16x3<a{a},n{n},e{e}>" if mode == "split3" else "gemm_f32<a{a},n{n},e{e}>")
    k_in = "gemm_bf16_patchin4" if bf_in else gen.format(a=2, n=0, e=0)
    k_out = "gemm_x3_astat<e4>" if x3_out else ("gemm_bf16_unpatch4" if bf_out else gen.format(a=0, n=1, e=4))
    src_in = "patch_bf16.hip" if bf_in else ("gemm_bf16.hip" if bf else "gemm.hip")
    src_out = "gemm_x3.hip" if x3_out else ("patch_bf16.hip" if bf_out else ("gemm_bf16.hip" if bf else "gemm.hip"))
    tag = f"{'bf16' if bf else mode},C{Cc},{H}x{W},p{p},d{d}{',sigma' if sigma else ''}"
    sig = torch.tensor([0.05, 1.3, 70.0])[:B]

    @case(f"patch_in[{tag}]", "patch_in", src_in, mode=None if bf else mode, kernel=k_in)
    def _(ops):
        ins = {"img": rn(B, Cc, H, W, seed=1), "w": rn(d, Cc * p * p, seed=2)}
        if sigma:
            ins["sigma"] = sig

        def ref(R):
            img = R["img"] * (solvers.karras_scalings(R["sigma"], 0.5)[2].view(-1, 1, 1, 1) if sigma else 1.0)
            return hdit.token_merge((rt(img) if bf else img).movedim(1, -1).contiguous(), wr(R["w"]), p, p)
        return dict(ins=ins, outs={"y": ((B, H // p, W // p, d), dt)}, ref=ref, tol=tol,
                    call=lambda T: ops.patch_in(T["img"], T["w"], (p, p), sigma=T.get("sigma"), sigma_data=0.5, out=T["y"], precision=nat.PREC_BF16 if bf else None))

    @case(f"patch_out[{tag}]", "patch_out", src_out, mode=None if bf else mode, kernel=k_out)
    def _(ops):
        ins = {"x": rn(B, H // p, W // p, d, seed=3).to(dt), "s": 1 + 0.1 * rn(d, seed=4), "w": rn(Cc * p * p, d, seed=5) / d ** 0.5}
        if sigma:
            ins["img"], ins["sigma"] = rn(B, Cc, H, W, seed=1), sig

        def ref(R):
            inner = hdit.token_split(rms(R["x"], R["s"]), wr(R["w"]), p, p).movedim(-1, 1)
            if not sigma:
                return inner
            c_skip, c_out, _ = solvers.karras_scalings(R["sigma"], 0.5)
            return inner * c_out.view(-1, 1, 1, 1) + R["img"] * c_skip.view(-1, 1, 1, 1)
        return dict(ins=ins, outs={"y": ((B, Cc, H, W), F32)}, ref=ref, tol=tol,
                    call=lambda T: ops.patch_out(T["x"], T["s"], T["w"], (p, p), Cc, x_in=T.get("img"), sigma=T.get("sigma"), sigma_data=0.5, out=T["y"]))


for _sig in (False, True):
    for _shape in [(1, 28, 28, 4, 64), (3, 16, 16, 2, 128)]:
        _patch(*_shape, "exact", sigma=_sig)
        _patch(*_shape, "split3", sigma=_sig)
        _patch(*_shape, None, bf=True, sigma=_sig)
    _patch(3, 72, 88, 4, 128, "split3", sigma=_sig)
    _patch(3, 72, 88, 4, 128, None, bf=True, sigma=_sig)


# ---- attention cores (test_attn_global_sizes, test_window_attention_*: gtol; test_attn_na2d_sizes, the split-stored tests and the streaming
# core: 1e-4; test_bf16_attention_cores: 1.2e-2; test_qk_prep_inplace: 2e-6) --------------------------------------------------------------------

def _attn(op, H, W, nh, B, mode, prep=None, bf=False, arg=(), tol=None, src=None, kernel=None):
    """prep: None (prepared q, k), "fly" ((scale_h, cos, sin) applied on the fly) or "packed" (split-stored operands)"""
    tol = tol or (1.2e-2 if bf else (1e-4 if op == "attn_na2d" or prep == "packed" else GTOL[mode]))
    src = src or ("attn_bf16.hip" if bf else ("attn_x3.hip" if prep == "packed" else "attn_f32.hip"))
    name = f"{op}[{'bf16' if bf else mode},{H}x{W},nh{nh},B{B}{''.join(f',{a}' for a in arg)},prep={prep}]"
    if kernel is None:          # global / window: one launch name per arithmetic; the split-stored global core of attn_x3.hip has its own
        kernel = op + ("_bf16" if bf else ("_f32" if mode == "exact" else ("_x3" if prep == "packed" and op == "attn_global" else "_bf16x3")))

    @case(name, op, src, mode=None if bf else mode, kernel=kernel)
    def _(ops):
        dt = BF if bf else F32
        q, k, v = (rn(B, H, W, nh, 64, seed=s, scale=sc) for s, sc in ((1, 0.6), (2, 0.6), (3, 1.0)))
        if bf:
            q, k, v = rt(q), rt(k), rt(v)
        ins = {"qkv": (pack(split_stored(q), split_stored(k), split_stored(v)) if prep == "packed" else pack(q, k, v)).to(dt)}
        if prep == "fly":
            ins["sh"] = torch.linspace(5.0, 12.0, nh)
            ins["cos"], ins["sin"] = tables(H, W, nh)
        shape = (B, H * W, nh * 64) if op == "attn_global" else (B, H, W, nh * 64)
        if op == "attn_global":
            ins["qkv"] = ins["qkv"].view(B, H * W, -1)

        def call(T):
            p = (T["sh"], T["cos"], T["sin"]) if prep == "fly" else prep
            return getattr(ops, op)(T["qkv"], nh, *arg, prep=p, out=T["y"])

        def ref(R):
            q64, k64, v64 = q.double(), k.double(), v.double()
            if prep == "fly":
                theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
                q64, k64 = hdit.cosine_sim_scale(q64, k64, R["sh"])
                q64, k64 = hdit.apply_rope(q64, theta), hdit.apply_rope(k64, theta)
            if op == "attn_global":
                return hdit.attn_global(q64.reshape(B, 1, H * W, nh, 64), k64.reshape(B, 1, H * W, nh, 64), v64.reshape(B, 1, H * W, nh, 64), 1.0).reshape(shape)
            if op == "attn_window":
                return hdit.attn_shifted_window(q64, k64, v64, arg[0], arg[1], 1.0).reshape(shape)
            return hdit.na2d(q64, k64, v64, arg[0], 1.0).reshape(shape)
        return dict(ins=ins, outs={"y": (shape, dt)}, call=call, ref=ref, tol=tol)


for _T, _nh, _B in [(7, 1, 1), (49, 4, 3), (100, 1, 2)]:
    for _mode in ("exact", "split3"):
        _attn("attn_global", 1, _T, _nh, _B, _mode)
    _attn("attn_global", 1, _T, _nh, _B, None, bf=True)
    _attn("attn_global", 1, _T, _nh, _B, "split3", prep="fly")
_attn("attn_global", 7, 7, 4, 3, "split3", prep="fly")
_attn("attn_global", 8, 8, 2, 2, "split3", prep="packed", kernel="attn_global_x3")
_attn("attn_global", 17, 16, 1, 3, "split3", tol=1e-4)
_attn("attn_global", 17, 16, 1, 3, "split3", prep="fly", tol=1e-4)
_attn("attn_global", 17, 16, 1, 3, None, bf=True)
for _H, _W, _ws, _shift in [(8, 24, 8, 4), (8, 12, 4, 2), (16, 32, 16, 8)]:
    for _mode in ("exact", "split3"):
        _attn("attn_window", _H, _W, 1, 2, _mode, arg=(_ws, _shift))
    _attn("attn_window", _H, _W, 1, 2, "split3", arg=(_ws, _shift), prep="fly")
    _attn("attn_window", _H, _W, 1, 2, "split3", arg=(_ws, _shift), prep="packed", src="attn_f32.hip")
    _attn("attn_window", _H, _W, 1, 2, None, bf=True, arg=(_ws, _shift))
for _H, _W, _nh, _B in [(7, 7, 1, 2), (20, 13, 1, 1)]:
    for _mode in ("exact", "split3"):
        _attn("attn_na2d", _H, _W, _nh, _B, _mode, arg=(7,), kernel="attn_na2d ")
    _attn("attn_na2d", _H, _W, _nh, _B, "split3", arg=(7,), prep="fly", kernel="attn_na2d ")
for _ks, _H, _W in [(3, 3, 5), (7, 7, 7), (5, 20, 13), (13, 13, 21), (11, 11, 13), (7, 14, 22)]:
    _attn("attn_na2d", _H, _W, 1, 2, "split3", arg=(_ks,), prep="packed", kernel="attn_na2d_x3")
    _attn("attn_na2d", _H, _W, 1, 2, None, bf=True, arg=(_ks,), kernel="attn_na2d_bf16")


@case("qk_prep_[B2,16x16,nh2]", "qk_prep_", "attn_f32.hip", kernel="qk_prep_f32")
def _(ops):
    B, H, W, nh = 2, 16, 16, 2
    ins = {"qkv": rn(B, H, W, 3 * nh * 64, seed=1), "sh": torch.tensor([9.0, 12.5])}
    ins["cos"], ins["sin"] = tables(H, W, nh)

    def ref(R):
        q, k, v = hdit.split_qkv(R["qkv"], nh)
        q, k = hdit.cosine_sim_scale(q, k, R["sh"])
        theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
        return pack(hdit.apply_rope(q, theta), hdit.apply_rope(k, theta), v)
    return dict(ins=ins, inplace=("qkv",), call=lambda T: ops.qk_prep_(T["qkv"], T["sh"], T["cos"], T["sin"], nh), ref=ref, tol=2e-6)


# ---- elementwise, solver steps (bit-exact against the oracle's fp32 rounding order: test_sampler_steps_bit_exact, test_dpm_solver_kernels,
# test_preconditioner_generic), conditioning front end, noise sources ---------------------------------------------------------------------------

def _ew(name, op, ins_fn, call, ref, tol=0, ref32=True, outs=None, inplace=(), src="elementwise.hip", mode=None):
    @case(name, op, src, mode=mode)
    def _(ops):
        return dict(ins=ins_fn(), outs=outs or {}, call=lambda T: call(ops, T), ref=ref, tol=tol, ref32=ref32, inplace=inplace)


_ew("rms_norm[37x96]", "rms_norm", lambda: {"x": rn(37, 96, seed=1), "s": 1 + 0.2 * rn(96, seed=2)}, lambda ops, T: ops.rms_norm(T["x"], T["s"], out=T["y"]),
    lambda R: rms(R["x"], R["s"]), tol=2e-6, ref32=False, outs={"y": ((37, 96), F32)})          # test_norm_linear_and_geglu: 2e-6

N_STEP = 513
_C = [0.731, -1.37, 1.618, 0.618]
_c = [torch.tensor(v, dtype=F32) for v in _C]


def _step_ins():
    return {"x": rn(N_STEP, seed=1, scale=30.0), "d": rn(N_STEP, seed=2), "o2": rn(N_STEP, seed=3), "a": rn(N_STEP, seed=4, scale=2.0)}


_STEPS = {
    "STEP_EULER": lambda R: R["x"] + ((R["x"] - R["d"]) / _c[0]) * _c[1],
    "STEP_DPMPP_2M1": lambda R: _c[0] * R["x"] - _c[1] * R["d"],
    "STEP_DPMPP_2M2": lambda R: _c[0] * R["x"] - _c[1] * (_c[2] * R["d"] - _c[3] * R["o2"]),
    "STEP_ADD_NOISE": lambda R: R["x"] + R["d"] * _C[0] * _c[1] * _c[2],
    "STEP_EULER_FROM": lambda R: R["x"] + ((R["o2"] - R["d"]) / _c[0]) * _c[1],
    "STEP_AXPBY": lambda R: _c[0] * R["x"] + _c[1] * R["d"],
    "STEP_ADD_DIFF": lambda R: R["x"] + _c[0] * (R["d"] - R["o2"]),
    "STEP_TO_D": lambda R: (R["x"] - R["d"]) / _c[0],
    "STEP_LERP2": lambda R: _c[0] * R["d"] + _c[1] * R["o2"],
    "STEP_AXPY": lambda R: R["x"] + R["d"] * _c[0],
}
for _name, _ref in _STEPS.items():
    _ew(f"sampler_step[{_name},n513]", "sampler_step", _step_ins,
        lambda ops, T, code=getattr(nat, _name): ops.sampler_step(code, T["x"], T["d"], in2=T["o2"], out=T["y"], c0=_C[0], c1=_C[1], c2=_C[2], c3=_C[3]),
        _ref, outs={"y": ((N_STEP,), F32)})


def _heun_pred(ops, T):
    y = ops.sampler_step(nat.STEP_HEUN_PRED, T["x"], T["d"], out=T["y"], aux=T["aux"], c0=_C[0], c1=_C[1])
    return y, T["aux"]


_ew("sampler_step[STEP_HEUN_PRED,aux written,n513]", "sampler_step", _step_ins, _heun_pred,
    lambda R: (R["x"] + ((R["x"] - R["d"]) / _c[0]) * _c[1], (R["x"] - R["d"]) / _c[0]), outs={"y": ((N_STEP,), F32), "aux": ((N_STEP,), F32)})
_ew("sampler_step[STEP_HEUN_CORR,aux read,n513]", "sampler_step", _step_ins,
    lambda ops, T: ops.sampler_step(nat.STEP_HEUN_CORR, T["x"], T["d"], in2=T["o2"], out=T["y"], aux=T["a"], c0=_C[0], c1=_C[1]),
    lambda R: R["x"] + ((R["a"] + (R["o2"] - R["d"]) / _c[0]) / 2) * _c[1], outs={"y": ((N_STEP,), F32)})
_ew("sampler_step[STEP_DPMPP_2M1,inplace,n513]", "sampler_step", _step_ins,
    lambda ops, T: ops.sampler_step(nat.STEP_DPMPP_2M1, T["x"], T["d"], out=T["x"], c0=_C[0], c1=_C[1]), _STEPS["STEP_DPMPP_2M1"], inplace=("x",))

_SIG3 = torch.tensor([0.01, 2.0, 160.0])


def _pc(R):
    return [c.view(-1, 1, 1, 1) for c in solvers.karras_scalings(R["sigma"], 0.5)]


def _img_ins():
    return {"x": rn(3, 3, 5, 7, seed=1, scale=20.0), "f": rn(3, 3, 5, 7, seed=2), "sigma": _SIG3.clone(), "a": rn(3, seed=5), "c": rn(3, seed=6)}


_IMG = {"y": ((3, 3, 5, 7), F32)}
_ew("precond_in[3x3x5x7]", "precond_in", _img_ins, lambda ops, T: ops.precond_in(T["x"], T["sigma"], 0.5, out=T["y"]), lambda R: R["x"] * _pc(R)[2], outs=_IMG)
_ew("precond_out[3x3x5x7]", "precond_out", _img_ins, lambda ops, T: ops.precond_out(T["f"], T["x"], T["sigma"], 0.5, out=T["y"]),
    lambda R: R["f"] * _pc(R)[1] + R["x"] * _pc(R)[0], outs=_IMG)
# rows_affine has no kernel-level test of its own: fp32 multiply-add of fp32 operands against fp64 -- 2 roundings of 2^-24 each: 2^-22
_ew("rows_affine[3x3x5x7]", "rows_affine", _img_ins, lambda ops, T: ops.rows_affine(T["f"], T["a"], x=T["x"], c=T["c"], out=T["y"]),
    lambda R: R["f"] * R["a"].view(-1, 1, 1, 1) + R["x"] * R["c"].view(-1, 1, 1, 1), tol=2.0 ** -22, ref32=False, outs=_IMG)
_ew("rows_affine[no x,3x3x5x7]", "rows_affine", _img_ins, lambda ops, T: ops.rows_affine(T["f"], T["a"], out=T["y"]),
    lambda R: R["f"] * R["a"].view(-1, 1, 1, 1), tol=2.0 ** -22, ref32=False, outs=_IMG)


def _dpm_ins():
    x, d = rn(N_STEP, seed=1, scale=30.0), rn(N_STEP, seed=2)
    return {"x": x, "d": d, "eps": (x - d) / _c[0], "e2": rn(N_STEP, seed=3, scale=5.0)}


_ew("dpm_eps[n513]", "dpm_eps", _dpm_ins, lambda ops, T: ops.dpm_eps(T["x"], T["d"], _C[0], out=T["y"]), lambda R: (R["x"] - R["d"]) / _c[0], outs={"y": ((N_STEP,), F32)})
_ew("dpm_combine[n513]", "dpm_combine", _dpm_ins, lambda ops, T: ops.dpm_combine(T["x"], T["eps"], _C[2], out=T["y"]), lambda R: R["x"] - _c[2] * R["eps"],
    outs={"y": ((N_STEP,), F32)})
_ew("dpm_combine[eps_r,n513]", "dpm_combine", _dpm_ins, lambda ops, T: ops.dpm_combine(T["x"], T["eps"], _C[2], T["e2"], _C[3], out=T["y"]),
    lambda R: R["x"] - _c[2] * R["eps"] - _c[3] * (R["e2"] - R["eps"]), outs={"y": ((N_STEP,), F32)})


def _dpm_error_ref(R):
    delta = torch.maximum(torch.tensor(0.0078, dtype=F32), torch.tensor(0.05, dtype=F32) * torch.maximum(R["lo"].abs(), R["prev"].abs()))
    return torch.linalg.norm(((R["lo"] - R["hi"]) / delta).double()) / R["lo"].numel() ** 0.5


_ew("dpm_error[3x5x7x11]", "dpm_error", lambda: {"lo": rn(3, 5, 7, 11, seed=5, scale=4.0), "hi": rn(3, 5, 7, 11, seed=6, scale=4.0), "prev": rn(3, 5, 7, 11, seed=7, scale=9.0)},
    lambda ops, T: ops.dpm_error(T["lo"], T["hi"], T["prev"], 0.0078, 0.05), _dpm_error_ref, tol=1e-6)          # test_dpm_solver_kernels: 1e-6 relative


def _ls():
    return torch.linspace(-3.0, 4.0, 37)


def _sigma_to_t_ref(quantize):
    def ref(R):
        ls, s = R["ls"], R["sigma"].log()
        dists = s - ls[:, None]
        if quantize:
            return dists.abs().argmin(0).double()
        low = dists.ge(0).cumsum(0).argmax(0).clamp(max=ls.numel() - 2)
        w = ((ls[low] - s) / (ls[low] - ls[low + 1])).clamp(0, 1)
        return (1 - w) * low + w * (low + 1)
    return ref


def _t_to_sigma_ref(R):
    t, ls = R["t"], R["ls"]
    low, high, w = t.floor().long(), t.ceil().long(), t.frac()
    return ((1 - w) * ls[low] + w * ls[high]).exp()


# tests/test_model_gpu.py (the wrappers' known-answer test): 1e-5, quantised bit-exact
_ew("sigma_to_t[n13]", "sigma_to_t", lambda: {"sigma": torch.logspace(-1.2, 1.6, 13), "ls": _ls()}, lambda ops, T: ops.sigma_to_t(T["sigma"], T["ls"], False),
    _sigma_to_t_ref(False), tol=1e-5, ref32=False)
_ew("sigma_to_t[quantize,n13]", "sigma_to_t", lambda: {"sigma": torch.logspace(-1.2, 1.6, 13) * 1.01, "ls": _ls()}, lambda ops, T: ops.sigma_to_t(T["sigma"], T["ls"], True),
    _sigma_to_t_ref(True), tol=0, ref32=False)
_ew("t_to_sigma[n13]", "t_to_sigma", lambda: {"t": torch.linspace(0.0, 36.0, 13) * 0.99, "ls": _ls()}, lambda ops, T: ops.t_to_sigma(T["t"], T["ls"]), _t_to_sigma_ref,
    tol=1e-5, ref32=False)

# test_conditioning_front_end: absolute 2e-5 / 5e-5 / 1e-6
_ew("fourier_sigma[B4,half128]", "fourier_sigma", lambda: {"sigma": torch.tensor([0.01, 0.3, 7.0, 160.0]), "w": rn(128, 1, seed=1)},
    lambda ops, T: ops.fourier_sigma(T["sigma"], T["w"], out=T["y"]), lambda R: hdit.fourier_features((torch.log(R["sigma"]) / 4)[:, None], R["w"]),
    tol=("abs", 2e-5), ref32=False, outs={"y": ((4, 256), F32)})
_ew("fourier_features[B5,in9,half127]", "fourier_features", lambda: {"x": rn(5, 9, seed=2, scale=0.3), "w": rn(127, 9, seed=3)},
    lambda ops, T: ops.fourier_features(T["x"], T["w"], out=T["y"]), lambda R: hdit.fourier_features(R["x"], R["w"]), tol=("abs", 5e-5), ref32=False,
    outs={"y": ((5, 254), F32)})
_ew("cond_sum[ids,B4,d256]", "cond_sum", lambda: {"a": rn(4, 256, seed=4), "b": rn(256, seed=5), "emb": rn(11, 256, seed=6), "c": rn(4, 256, seed=7), "ids": torch.tensor([10, 0, 3, 3])},
    lambda ops, T: ops.cond_sum(T["a"], T["b"], T["emb"], T["ids"], T["c"], out=T["y"]), lambda R: R["a"] + R["b"] + R["emb"][R["ids"]] + R["c"],
    tol=("abs", 1e-6), ref32=False, outs={"y": ((4, 256), F32)})
_ew("cond_sum[no ids,B3,d100]", "cond_sum", lambda: {"a": rn(3, 100, seed=4), "c": rn(3, 100, seed=7)}, lambda ops, T: ops.cond_sum(T["a"], T["c"], out=T["y"]),
    lambda R: R["a"] + R["c"], tol=("abs", 1e-6), ref32=False, outs={"y": ((3, 100), F32)})
# (x in [-1.5, 1.5) so that no reference byte is 0xFF, the pre-fill of a uint8 output: an unwritten byte then fails the exact comparison)
_ew("to_uint8[n1001]", "to_uint8", lambda: {"x": torch.linspace(-1.5, 0.99, 1001)}, lambda ops, T: ops.to_uint8(T["x"], out=T["y"]),
    lambda R: (((R["x"].clamp(-1, 1) + 1) / 2) * 255).to(U8), tol=0, outs={"y": ((1001,), U8)})

_SEEDS = [12345, 2 ** 63 - 7, 0]


def _seeds():
    return {"seeds": torch.tensor(_SEEDS, dtype=I64)}


# test_brownian_vs_oracle: 1e-4 absolute; test_index_addressed_normals_vs_oracle: 1e-5 absolute per unit of scale
_ew("brownian[3x3x5x7]", "brownian", _seeds, lambda ops, T: ops.brownian(T["y"], T["seeds"], 0.01, 80.0, 0.5, 3.25, 0.6),
    lambda R: torch.from_numpy(obrown.brownian_increment(_SEEDS, 105, 0.01, 80.0, 0.5, 3.25, 0.6)), tol=("abs", 1e-4), outs={"y": ((3, 3, 5, 7), F32)}, src="brownian.hip")
_ew("randn_indexed[3x3x5x7]", "randn_indexed", _seeds, lambda ops, T: ops.randn_indexed(T["y"], T["seeds"], draw=3, scale=1.0),
    lambda R: torch.from_numpy(obrown.randn_indexed(_SEEDS, 105, draw=3, scale=1.0)), tol=("abs", 1e-5), outs={"y": ((3, 3, 5, 7), F32)}, src="brownian.hip")


def _bc(ops, T):
    ops.brownian_cached(T["y"], T["w0"], False, T["w1"], False, T["seeds"], 0.01, 80.0, 1.0, 2.0, 0.7)      # fills W(1), W(2)
    return T["y"], T["w0"], T["w1"]


def _bc_ref(R):
    w = [torch.from_numpy(np.stack([obrown.brownian_w(s & (2 ** 64 - 1), 105, t, 0.01, 80.0) for s in _SEEDS])) for t in (1.0, 2.0)]
    return torch.from_numpy(obrown.brownian_increment(_SEEDS, 105, 0.01, 80.0, 1.0, 2.0, 0.7)), w[0], w[1]


_ew("brownian_cached[fill both,3x105]", "brownian_cached", _seeds, _bc, _bc_ref, tol=("abs", 1e-4), outs={k: ((3, 105), F32) for k in ("y", "w0", "w1")}, src="brownian.hip")


def _bc_read(ops, T):
    return ops.brownian_cached(T["y"], T["w0"], True, T["w1"], True, T["seeds"], 0.01, 80.0, 1.0, 2.0, -2.0)


_ew("brownian_cached[read both,3x105]", "brownian_cached", lambda: dict(_seeds(), w0=rn(3, 105, seed=1), w1=rn(3, 105, seed=2)), _bc_read,
    lambda R: (R["w1"].double() - R["w0"].double()) * -2.0, tol=2.0 ** -22, outs={"y": ((3, 105), F32)}, src="brownian.hip")       # one subtraction, one product in fp32


# ---- forward- and reverse-mode kernels (tests/test_likelihood_gpu.py, tests/test_vjp_gpu.py: KTOL = 1e-5 against fp64) -------------------------
KTOL = 1e-5


def _vjp64(f, x, gy):
    x64 = x.double().requires_grad_()
    with torch.enable_grad():
        gx, = torch.autograd.grad(f(x64), x64, gy.double())
    return gx


def _rmsnorm_d(rows, d, B, ada, vjp, add=False):
    @case(f"rms_norm_{'vjp' if vjp else 'jvp'}[rows{rows},d{d},B{B},{'ada' if ada else 'gain'}{',add,out' if add else ''}]", "rms_norm_vjp" if vjp else "rms_norm_jvp",
          "vjp_f32.hip" if vjp else "jvp_f32.hip")
    def _(ops):
        ins = {"x": rn(B, rows, d, seed=1), "t": rn(B, rows, d, seed=2), "s": ru(B, d, seed=3) + 0.5 if ada else ru(d, seed=3) + 0.5}
        if add:
            ins["add"] = rn(B, rows, d, seed=4)
        f = lambda R: (lambda u: rms(u, R["s"][:, None, :] if ada else R["s"]))
        if vjp:
            return dict(ins=ins, outs={"y": ((B, rows, d), F32)} if add else {}, tol=KTOL,
                        call=lambda T: ops.rms_norm_vjp(T["x"], T["t"], T["s"], rows_per_sample=rows, add=T.get("add"), out=T.get("y")),
                        ref=lambda R: _vjp64(f(R), R["x"], R["t"]) + (R["add"] if add else 0))
        return dict(ins=ins, call=lambda T: ops.rms_norm_jvp(T["x"], T["t"], T["s"], rows_per_sample=rows), ref=lambda R: fd_jvp(f(R), R["x"], R["t"]), tol=KTOL)


for _vjp in (False, True):
    _rmsnorm_d(7, 512, 1, False, _vjp)
    _rmsnorm_d(50, 256, 5, True, _vjp, add=_vjp)


def _geglu_d(vjp, drop=False):
    @case(f"geglu_{'vjp' if vjp else 'jvp'}[3x37x96{',dropout' if drop else ''}]", "geglu_vjp" if vjp else "geglu_jvp", "vjp_f32.hip" if vjp else "jvp_f32.hip")
    def _(ops):
        ins = {"h": rn(3, 37, 192, seed=1, scale=3.0), "t": rn(3, 37, 96 if vjp else 192, seed=2)}
        if drop:
            ins["key"] = torch.tensor([-3], dtype=I64)
        site, p = (1 << 62) | 5, 0.1
        if not vjp:
            return dict(ins=ins, call=lambda T: ops.geglu_jvp(T["h"], T["t"]), ref=lambda R: fd_jvp(geglu, R["h"], R["t"]), tol=KTOL)

        def ref(R):
            gy = R["t"]
            if drop:
                gy = (gy.float() * torch.from_numpy(np_mask(-3, site, p, gy.numel())).view(gy.shape)).double()        # the fp32 product the kernel forms
            return _vjp64(geglu, R["h"], gy)
        return dict(ins=ins, call=lambda T: ops.geglu_vjp(T["h"], T["t"], dropout=(T["key"], site, p) if drop else None), ref=ref, tol=KTOL)


_geglu_d(False)
_geglu_d(True)
_geglu_d(True, drop=True)


def _qk_prep_d(vjp):
    @case(f"qk_prep_{'vjp' if vjp else 'jvp'}_[B3,5x7,nh4]", "qk_prep_vjp_" if vjp else "qk_prep_jvp_", "vjp_f32.hip" if vjp else "jvp_f32.hip")
    def _(ops):
        B, H, W, nh = 3, 5, 7, 4
        ins = {"qkv": rn(B, H, W, 3 * nh * 64, seed=1), "t": rn(B, H, W, 3 * nh * 64, seed=2), "sh": torch.linspace(4.0, 12.0, nh)}
        ins["cos"], ins["sin"] = tables(H, W, nh)

        def f(R):
            def fn(u):
                q, k, v = hdit.split_qkv(u, nh)
                q, k = hdit.cosine_sim_scale(q, k, R["sh"])
                theta = hdit.rope_theta(hdit.axial_pos(H, W), hdit.rope_freqs(nh)).double()
                return pack(hdit.apply_rope(q, theta), hdit.apply_rope(k, theta), v)
            return fn
        if vjp:
            return dict(ins=ins, inplace=("t",), call=lambda T: ops.qk_prep_vjp_(T["qkv"], T["t"], T["sh"], T["cos"], T["sin"], nh),
                        ref=lambda R: _vjp64(f(R), R["qkv"], R["t"]), tol=KTOL)
        return dict(ins=ins, inplace=("qkv", "t"), call=lambda T: ops.qk_prep_jvp_(T["qkv"], T["t"], T["sh"], T["cos"], T["sin"], nh),
                    ref=lambda R: fd_jvp(f(R), R["qkv"], R["t"]), tol=KTOL)


_qk_prep_d(False)
_qk_prep_d(True)


def _attn_d(kind, vjp, B, H, W, nh, arg=()):
    op = f"attn_{kind}_{'vjp' if vjp else 'jvp'}"

    @case(f"{op}[B{B},{H}x{W},nh{nh}{''.join(f',{a}' for a in arg)}]", op, "vjp_f32.hip" if vjp else "jvp_f32.hip")
    def _(ops):
        q, k, v = (rn(B, H, W, nh, 64, seed=s) for s in (1, 2, 3))
        q, k = hdit.cosine_sim_scale(q, k, torch.full([nh], 10.0))
        ins = {"qkv": pack(q, k, v), "t": rn(B, H, W, nh * 64, seed=4) if vjp else rn(B, H, W, 3 * nh * 64, seed=4, scale=0.3)}
        fn = {"global": hdit.attn_global, "na2d": lambda a, b, c: hdit.na2d(a, b, c, arg[0]), "window": lambda a, b, c: hdit.attn_shifted_window(a, b, c, arg[0], arg[1])}[kind]

        def f(u):
            a, b, c = hdit.split_qkv(u, nh)
            return fn(a, b, c).reshape(B, H, W, nh * 64)
        call = lambda T: getattr(ops, op)(T["qkv"], T["t"], nh, *arg)
        if vjp:
            return dict(ins=ins, call=call, ref=lambda R: _vjp64(f, R["qkv"], R["t"]), tol=KTOL)
        return dict(ins=ins, call=call, ref=lambda R: fd_jvp(f, R["qkv"], R["t"]), tol=KTOL)


for _vjp in (False, True):
    _attn_d("global", _vjp, 1, 1, 3, 1)
    _attn_d("global", _vjp, 2, 7, 9, 2)
    _attn_d("na2d", _vjp, 2, 9, 11, 2, (3,))
    _attn_d("na2d", _vjp, 2, 13, 17, 2, (13,))
    _attn_d("window", _vjp, 2, 8, 12, 2, (4, 0))
    _attn_d("window", _vjp, 2, 8, 12, 2, (4, 2))


def _pcv(R):
    var = (R["sigma"] ** 2 + 0.25).view(-1, 1, 1, 1)
    return 0.25 / var, R["sigma"].view(-1, 1, 1, 1) * 0.5 / var.sqrt(), 1 / var.sqrt()


_ew("precond_vjp[PC_OUT,3x2x5x7]", "precond_vjp", lambda: {"g": rn(3, 2, 5, 7, seed=1), "sigma": torch.tensor([0.05, 1.0, 60.0])},
    lambda ops, T: ops.precond_vjp(T["g"], nat.PC_OUT, T["sigma"], 0.5, out=T["y"]), lambda R: R["g"] * _pcv(R)[1], tol=KTOL, ref32=False,
    outs={"y": ((3, 2, 5, 7), F32)}, src="vjp_f32.hip")
_ew("precond_vjp[PC_IN + PC_SKIP h,3x2x5x7]", "precond_vjp", lambda: {"g": rn(3, 2, 5, 7, seed=1), "h": rn(3, 2, 5, 7, seed=2), "sigma": torch.tensor([0.05, 1.0, 60.0])},
    lambda ops, T: ops.precond_vjp(T["g"], nat.PC_IN, T["sigma"], 0.5, h=T["h"], h_coef=nat.PC_SKIP, out=T["y"]), lambda R: R["g"] * _pcv(R)[2] + R["h"] * _pcv(R)[0],
    tol=KTOL, ref32=False, outs={"y": ((3, 2, 5, 7), F32)}, src="vjp_f32.hip")


# ---- weight gradients and the loss (tests/test_param_grad_gpu.py: _bounds -- 1e-6 exact up to 1024 rows, 3e-6 beyond, 2e-5 split3; colsum 1e-5,
# row_rrms / attn_scale_grad / class_emb_grad 1e-6, loss kernels 1e-6 / 1e-5; tests/test_wgrad_bf16_gpu.py for the bf16 operands) ----------------

def _wbound(mode, M):
    return {"exact": 1e-6 if M <= 1024 else 3e-6, "split3": 2e-5}[mode]


WG_KERNEL = {"exact": "wgrad_f32", "split3": "wgrad_x3_f32", "bf16": "wgrad_b16_f32"}


def _device_geglu(ops, U):
    """value * gelu(gate) in fp32 as the device evaluates it (tests/test_wgrad_bf16_gpu.py: _device_geglu): read back through the exact-fp32
    weight gradient of an identity G -- every sum is one operand element times 1.0 plus zeros.  The device's erff and the CPU's erf differ in
    the last fp32 bit on some elements, and such an element next to a bf16 rounding boundary rounds the other way; so the bf16 form's operand
    'after its prologue' is the device's fp32 value, held to the CPU's GEGLU within fp32 rounding here."""
    dev = ops.wgrad(torch.eye(U.shape[0], device=DEV), U.to(DEV), geglu=True, precision=nat.PREC_EXACT).cpu()
    cpu = geglu(U)
    d = U.shape[-1] // 2
    scale = cpu.abs() + (U[:, :d] * U[:, d:]).abs()
    assert ((dev - cpu).abs() <= 4e-7 * scale).all()
    return dev


def _b16_rule(box):
    """tests/test_wgrad_bf16_gpu.py: _check -- max|hip - fp64| <= 4 max|torch fp32 - fp64| on the product of the bf16-rounded operands"""
    def tol(got, ref):
        e_hip, e_yard = (got.detach().cpu().double() - ref).abs().max().item(), (box["yard"].double() - ref).abs().max().item()
        assert e_hip <= 4 * e_yard, f"max|hip - fp64| {e_hip:.3e} > 4 x max|torch fp32 - fp64| {e_yard:.3e}"
        return e_hip
    return tol


def _b16_truth(box, Gop, Aop, base=None, alpha=None):
    """fp64 product of the bf16-rounded fp32 operands (after their prologue, in fp32 as the kernel forms them); the fp32 yardstick goes into box"""
    Gb, Ab = Gop.bfloat16(), Aop.bfloat16()
    truth, yard = Gb.double().T @ Ab.double(), Gb.float().T @ Ab.float()
    if base is not None:
        truth, yard = base.double() + float(alpha) * truth, base + alpha * yard
    box["yard"] = yard
    return truth


def _wgrad(M, mode, variant="plain", N=96, K=40):
    bf = mode == "bf16"
    box = {}            # (outlives make(): the references are computed once and shared by the two fills)

    @case(f"wgrad[{variant},{mode},M{M},N{N},K{K}]", "wgrad", "wgrad_f32.hip", mode="split3" if bf else mode, kernel=WG_KERNEL[mode])
    def _(ops):
        B = 1 if M < 4 or M % 2 else 2
        rps = M // B
        ins = {"G": rn(M, N, seed=1), "A": rn(M, 2 * K if variant == "geglu" else K, seed=2, scale=2.0 if variant == "geglu" else 1.0)}
        outs, inplace = {"y": ((N, K), F32)}, ()
        if variant == "accumulate":
            ins["acc"], ins["alpha"] = rn(N, K, seed=3), torch.tensor([0.75])
            outs, inplace = {}, ("acc",)
        if variant == "scales":
            ins["rr"], ins["cs"] = ru(M, seed=4) + 0.5, ru(B, K, seed=5) + 0.5

        def call(T):
            if variant == "accumulate":
                return ops.wgrad(T["G"], T["A"], out=T["acc"], accumulate=True, alpha=T["alpha"], bf16=bf)
            if variant == "scales":
                return ops.wgrad(T["G"], T["A"], out=T["y"], row_scale=T["rr"], col_scale=T["cs"], rows_per_sample=rps, bf16=bf)
            return ops.wgrad(T["G"], T["A"], out=T["y"], geglu=variant == "geglu", bf16=bf)

        def ref(R):
            a = R["A"]
            if bf:                                   # R holds the fp32 inputs (ref32): the prologue in fp32, as the kernel and the existing test form it
                if variant == "geglu":
                    a = _device_geglu(ops, a)
                if variant == "scales":
                    a = (a * R["rr"][:, None]) * R["cs"].repeat_interleave(rps, 0)
                return _b16_truth(box, R["G"], a, R.get("acc") if variant == "accumulate" else None, R.get("alpha"))
            if variant == "geglu":
                a = geglu(a)
            if variant == "scales":
                a = a * R["rr"][:, None] * R["cs"].repeat_interleave(rps, 0)
            y = R["G"].T @ a
            return R["acc"] + 0.75 * y if variant == "accumulate" else y
        return dict(ins=ins, outs=outs, inplace=inplace, call=call, ref=ref, ref32=bf, tol=_b16_rule(box) if bf else _wbound(mode, M))


for _M in (1, 3, 37, 4113):
    for _mode in ("exact", "split3", "bf16"):
        _wgrad(_M, _mode)
for _mode in ("exact", "split3", "bf16"):
    for _variant in ("accumulate", "scales", "geglu"):
        _wgrad(37, _mode, _variant)
        _wgrad(4113 if _variant != "geglu" or _mode != "bf16" else 1029, _mode, _variant, N=128, K=64)     # (the identity G of _device_geglu is M x M)


def _wgrad_gather(kind, which, mode):
    bf = mode == "bf16"
    box = {}

    @case(f"wgrad[{kind} gather on {which},{mode}]", "wgrad", "wgrad_f32.hip", mode="split3" if bf else mode, kernel=WG_KERNEL[mode])
    def _(ops):
        if kind == "merge":
            B, gh, gw, Cc, N = 3, 5, 7, 128, 96
            fine = rn(B, 2 * gh, 2 * gw, Cc, seed=1)
            rows = lambda t: t.view(B, gh, 2, gw, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, 4 * Cc)
            geom, code = (gh, gw, 2, 2, Cc), nat.WG_MERGE2x2
        else:
            B, Cc, H, W, ph, N = 3, 1, 28, 28, 4, 128
            gh, gw = H // ph, W // ph
            fine = rn(B, Cc, H, W, seed=1)
            rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, gh, ph, gw, ph, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, ph * ph * Cc)
            geom, code = (gh, gw, ph, ph, Cc), nat.WG_PATCH_NCHW
        ins = {"fine": fine, "X": rn(B * gh * gw, N, seed=2)}
        kdim = geom[2] * geom[3] * Cc
        tol = _b16_rule(box) if bf else _wbound(mode, 1)
        prod = (lambda g_, a_: _b16_truth(box, g_, a_)) if bf else (lambda g_, a_: g_.T @ a_)
        if which == "a":
            return dict(ins=ins, outs={"y": ((N, kdim), F32)}, call=lambda T: ops.wgrad(T["X"], T["fine"], gather=("a", code), gather_geom=geom, out=T["y"], bf16=bf),
                        ref=lambda R: prod(R["X"], rows(R["fine"])), ref32=bf, tol=tol)
        return dict(ins=ins, outs={"y": ((kdim, N), F32)}, call=lambda T: ops.wgrad(T["fine"], T["X"], gather=("g", code), gather_geom=geom, out=T["y"], bf16=bf),
                    ref=lambda R: prod(rows(R["fine"]), R["X"]), ref32=bf, tol=tol)


for _kind in ("merge", "patch"):
    for _which in ("a", "g"):
        for _mode in ("exact", "split3", "bf16"):
            _wgrad_gather(_kind, _which, _mode)


def _colsum(rows, cols, seg, acc):
    @case(f"colsum[rows{rows},cols{cols},seg{seg}{',accumulate' if acc else ''}]", "colsum", "wgrad_f32.hip")
    def _(ops):
        ins = {"a": rn(rows, cols, seed=1)}
        if acc:
            ins["acc"] = rn(rows // seg, cols, seed=5)
            return dict(ins=ins, inplace=("acc",), call=lambda T: ops.colsum(T["a"], rows_per_seg=seg, out=T["acc"], accumulate=True),
                        ref=lambda R: R["acc"] + R["a"].view(rows // seg, seg, cols).sum(1), tol=1e-5)
        ins.update(b=rn(rows, cols, seed=2), b2=rn(rows, cols, seed=3), rs=ru(rows, seed=4) + 0.5)
        return dict(ins=ins, outs={"y": ((rows // seg, cols), F32)}, call=lambda T: ops.colsum(T["a"], T["b"], T["b2"], row_scale=T["rs"], rows_per_seg=seg, out=T["y"]),
                    ref=lambda R: (R["a"] * (R["b"] - R["b2"]) * R["rs"][:, None]).view(rows // seg, seg, cols).sum(1), tol=1e-5)


_colsum(37, 768, 37, False)
_colsum(195, 100, 65, False)
_colsum(195, 100, 65, True)
_colsum(1, 256, 1, False)

_ew("row_rrms[37x100]", "row_rrms", lambda: {"x": rn(37, 100, seed=1)}, lambda ops, T: ops.row_rrms(T["x"]), lambda R: torch.rsqrt(R["x"].pow(2).mean(-1) + 1e-6),
    tol=1e-6, ref32=False, src="wgrad_f32.hip")
_ew("attn_scale_grad[nh4]", "attn_scale_grad", lambda: {"cs": rn(768, seed=1), "sh": ru(4, seed=2) * 10 + 1}, lambda ops, T: ops.attn_scale_grad(T["cs"], T["sh"], 4, out=T["y"]),
    lambda R: R["cs"].view(3, 4, 64)[:2].sum((0, 2)) / (2 * R["sh"]), tol=1e-6, ref32=False, outs={"y": ((4,), F32)}, src="wgrad_f32.hip")
_ew("class_emb_grad[B7,d256,n11]", "class_emb_grad", lambda: {"g": rn(7, 256, seed=1), "ids": torch.tensor([3, 0, 3, 10, 1, 3, 0])},
    lambda ops, T: ops.class_emb_grad(T["g"], T["ids"], 11, out=T["y"]), lambda R: torch.zeros(11, 256, dtype=F64).index_add_(0, R["ids"], R["g"]), tol=1e-6, ref32=False,
    outs={"y": ((11, 256), F32)}, src="wgrad_f32.hip")


def _loss_ins():
    x, n, sigma = rn(3, 3, 5, 7, seed=1), rn(3, 3, 5, 7, seed=2), torch.tensor([0.05, 1.3, 40.0])
    return {"x": x, "n": n, "f": rn(3, 3, 5, 7, seed=3), "sigma": sigma, "noised": x + n * sigma.view(-1, 1, 1, 1), "cw": torch.tensor([0.7, 1.9, 0.05]),
            "gl": torch.tensor([0.3, -1.0, 2.0])}


def _loss_ref(R, code):
    s = R["sigma"].view(-1, 1, 1, 1)
    var = s ** 2 + 0.25
    c_skip, c_out = 0.25 / var, s * 0.5 / var.sqrt()
    w = [torch.ones(3, dtype=F64), (R["sigma"] * 0.5) ** 2 / (R["sigma"] ** 2 + 0.25) ** 2, 0.25 / (R["sigma"] ** 2 + 0.25), R["cw"]][code]
    return lambda f: ((f - (R["x"] - c_skip * R["noised"]) / c_out) ** 2).flatten(1).mean(1) * w


def _loss_prep_ref(R):
    nz = R["x"] + R["n"] * R["sigma"].view(-1, 1, 1, 1)
    return nz, nz / (R["sigma"].view(-1, 1, 1, 1) ** 2 + 0.25).sqrt()


_ew("loss_prep[3x3x5x7]", "loss_prep", _loss_ins, lambda ops, T: ops.loss_prep(T["x"], T["n"], T["sigma"], 0.5), _loss_prep_ref, tol=1e-6, ref32=False, src="wgrad_f32.hip")
for _code, _wname in enumerate(("karras", "soft-min-snr", "snr", "given")):
    _ew(f"loss[{_wname},3x3x5x7]", "loss", _loss_ins, lambda ops, T, c=_code: ops.loss(T["f"], T["x"], T["noised"], T["sigma"], 0.5, c, T["cw"] if c == 3 else None),
        lambda R, c=_code: _loss_ref(R, c)(R["f"]), tol=1e-5, ref32=False, src="wgrad_f32.hip")
    _ew(f"loss_vjp[{_wname},3x3x5x7]", "loss_vjp", _loss_ins,
        lambda ops, T, c=_code: ops.loss_vjp(T["f"], T["x"], T["noised"], T["sigma"], 0.5, c, T["gl"], T["cw"] if c == 3 else None),
        lambda R, c=_code: _vjp64(_loss_ref(R, c), R["f"], R["gl"]), tol=1e-5, ref32=False, src="wgrad_f32.hip")


# ---- dropout (tests/test_dropout_gpu.py: bit-exact against the restated mask contract) ------------------------------------------------------

def _dropout(n, inplace):
    key, site, p = 0x0123456789ABCDEF, (1 << 62) | (1 << 32) | 1, 0.1

    def ref(R):
        return R["x"] * torch.from_numpy(np_mask(key, site, p, n))
    _ew(f"dropout[n{n}{',inplace' if inplace else ''}]", "dropout", lambda: {"x": rn(n, seed=n, scale=3.0), "key": torch.tensor([key], dtype=I64)},
        lambda ops, T: ops.dropout(T["x"], T["key"], site, p, out=T["x"] if inplace else T["y"]), ref, tol=0, outs={} if inplace else {"y": ((n,), F32)},
        inplace=("x",) if inplace else (), src="dropout_f32.hip")


for _n in (1, 3, 1027):
    _dropout(_n, False)
_dropout(1027, True)


# ---- likelihood kernels (tests/test_likelihood_gpu.py: KTOL) ---------------------------------------------------------------------------------

def _ll_ins():
    x, D, Dd = (rn(3, 2, 9, 11, seed=s) for s in (1, 2, 3))
    return {"x": x, "D": D, "Dd": Dd, "v": (ru(3, 2, 9, 11, seed=4) > 0.5).float() * 2 - 1, "sigma": torch.tensor([0.1, 2.0, 70.0])}


_ew("ll_div[3x2x9x11]", "ll_div", _ll_ins, lambda ops, T: ops.ll_div(T["x"], T["D"], T["Dd"], T["v"], T["sigma"]),
    lambda R: ((R["x"] - R["D"]) / R["sigma"].view(-1, 1, 1, 1), (R["v"] * (R["v"] - R["Dd"])).flatten(1).sum(1) / R["sigma"]), tol=KTOL, ref32=False, src="jvp_f32.hip")
_ew("gauss_logp[3x2x9x11]", "gauss_logp", _ll_ins, lambda ops, T: ops.gauss_logp(T["x"], 3.5, add=T["sigma"]),
    lambda R: torch.distributions.Normal(0.0, 3.5).log_prob(R["x"]).flatten(1).sum(1) + R["sigma"], tol=KTOL, ref32=False, src="jvp_f32.hip")
_RKC = [0.3, -1.2, 0.0, 2.5, 0.1, -0.7, 1.0 / 60]


def _rk_ins():
    ins = {f"k{i}": rn(1001, seed=10 + i) for i in range(7)}
    ins.update(y0=rn(1001, seed=20), y1=rn(1001, seed=21))
    return ins


def _rk_err(R):
    return sum(c * R[f"k{i}"] for i, c in enumerate(_RKC)) / (1e-4 + 1e-3 * torch.maximum(R["y0"].abs(), R["y1"].abs()))


_ew("rk_combine[7 terms,n1001]", "rk_combine", _rk_ins, lambda ops, T: ops.rk_combine(T["y0"], [T[f"k{i}"] for i in range(7)], _RKC, out=T["y"]),
    lambda R: R["y0"] + sum(c * R[f"k{i}"] for i, c in enumerate(_RKC)), tol=KTOL, ref32=False, outs={"y": ((1001,), F32)}, src="jvp_f32.hip")
_ew("rk_error_partial[7 terms,n1001]", "rk_error_partial", _rk_ins,
    lambda ops, T: ops.rk_error_partial([T[f"k{i}"] for i in range(7)], _RKC, T["y0"], T["y1"], 1e-4, 1e-3).double().sum(),
    lambda R: _rk_err(R).pow(2).sum(), tol=1e-5, ref32=False, src="jvp_f32.hip")


# ---- metrics (tests/test_metrics_gpu.py: 3e-7 of the sum of the terms' magnitudes for the MMD, 3e-5 / 2e-6 per entry of the kernel matrix;
# the fp64 helpers against fp64 torch: a few fp64 ulps of the largest entry, 1e-13) --------------------------------------------------------------

def _poly(x, y):
    return (x @ y.transpose(-1, -2) / x.shape[-1] + 1) ** 3


def _mmd_ref(R):
    x, y = R["x"], R["y"]
    m, n = x.shape[-2], y.shape[-2]
    kxx, kyy, kxy = _poly(x, x), _poly(y, y), _poly(x, y)
    t1 = (kxx.sum((-1, -2)) - kxx.diagonal(dim1=-1, dim2=-2).sum(-1)) / (m * (m - 1))
    t2 = (kyy.sum((-1, -2)) - kyy.diagonal(dim1=-1, dim2=-2).sum(-1)) / (n * (n - 1))
    return t1 + t2 - 2 * kxy.mean((-1, -2)), t1.abs() + t2.abs() + 2 * kxy.mean((-1, -2)).abs()


for _mode in ("exact", "split3"):
    @case(f"mmd_poly[{_mode},B2,m67,n130,d37]", "mmd_poly", "metrics_f32.hip", mode=_mode)
    def _(ops):
        ins = {"x": ru(2, 67, 37, seed=1), "y": ru(2, 130, 37, seed=2) + 0.05}

        def ref(R):
            val, terms = _mmd_ref(R)
            return val / terms, None                      # measured in units of the terms, as the existing test does: bound 3e-7 absolute

        def call(T):
            got = ops.mmd_poly(T["x"], T["y"], out=T["o"])
            _, terms = _mmd_ref({k: v.detach().cpu().double() for k, v in T.items() if k in "xy"})
            return got.double() / terms.to(got.device), got
        return dict(ins=ins, outs={"o": ((2,), F32)}, call=call, ref=ref, tol=[("abs", 3e-7), None])

    @case(f"poly_kernel[{_mode},B2,m100,n130,d37]", "poly_kernel", "metrics_f32.hip", mode=_mode)
    def _(ops, mode=_mode):
        ins = {"x": ru(2, 100, 37, seed=1), "y": ru(2, 130, 37, seed=2)}
        # per-entry bound of the existing test; every entry lies in [1, 8], so per entry <= bound x 8 / max = the max-norm bound used here
        return dict(ins=ins, call=lambda T: ops.poly_kernel(T["x"], T["y"]), ref=lambda R: _poly(R["x"], R["y"]), tol=3e-5 if mode == "split3" else 2e-6)


def _mats_ins():
    x, y = ru(2, 67, 37, seed=1).double(), ru(2, 130, 37, seed=2).double()
    return {"kxx": _poly(x, x).float(), "kyy": _poly(y, y).float(), "kxy": _poly(x, y).float()}


def _mats_parts(R):
    t1 = (R["kxx"].sum((-1, -2)) - R["kxx"].diagonal(dim1=-1, dim2=-2).sum(-1)) / (67 * 66)
    t2 = (R["kyy"].sum((-1, -2)) - R["kyy"].diagonal(dim1=-1, dim2=-2).sum(-1)) / (130 * 129)
    return t1, t2, R["kxy"].mean((-1, -2))


def _mats_call(ops, T):
    t1, t2, t3 = _mats_parts({k: v.double() for k, v in T.items()})
    return ops.mmd_mats(T["kxx"], T["kyy"], T["kxy"]).double() / (t1 + t2 + 2 * t3)          # in units of the terms, as for mmd_poly


def _mats_ref(R):
    t1, t2, t3 = _mats_parts(R)
    return (t1 + t2 - 2 * t3) / (t1 + t2 + 2 * t3)


_ew("mmd_mats[B2,m67,n130]", "mmd_mats", _mats_ins, _mats_call, _mats_ref, tol=("abs", 3e-7), ref32=False, src="metrics_f32.hip")

F64TOL = 1e-13


def _m64(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _center_call(ops, T):
    return ops.center(T["x"])


_ew("center[67x37]", "center", lambda: {"x": rn(67, 37, seed=1)}, _center_call, lambda R: (R["x"] - R["x"].mean(0), R["x"].mean(0)), tol=[1e-6, 1e-6], ref32=False,
    src="metrics_f32.hip")          # fp32 column sums (colsum's 1e-5 is for cancelling products; plain sums of 67 terms: 1e-6)
_ew("gemm_tn_f64[b2,M37,N13,K21]", "gemm_tn_f64", lambda: {"G": _m64(2, 37, 13, seed=1), "A": _m64(2, 37, 21, seed=2), "rs": _m64(2, 37, seed=3)},
    lambda ops, T: ops.gemm_tn_f64(T["G"], T["A"], row_scale=T["rs"]), lambda R: R["G"].transpose(1, 2) @ (R["A"] * R["rs"][..., None]), tol=F64TOL, src="metrics_f32.hip")
_ew("gemm_tn_f64[out32,b2,M37,N13,K21]", "gemm_tn_f64", lambda: {"G": _m64(2, 37, 13, seed=1), "A": _m64(2, 37, 21, seed=2)},
    lambda ops, T: ops.gemm_tn_f64(T["G"], T["A"], out32=True), lambda R: R["G"].transpose(1, 2) @ R["A"], tol=2.0 ** -23, src="metrics_f32.hip")


def _sym_ref(R):
    low = torch.tril(R["a"].double())
    return low + torch.tril(low, -1).transpose(1, 2) + 0.5 * torch.eye(13, dtype=F64), torch.eye(13, dtype=F64).expand(2, 13, 13)


_ew("sym_lower_f64[b2,n13]", "sym_lower_f64", lambda: {"a": rn(2, 13, 13, seed=1)}, lambda ops, T: ops.sym_lower_f64(T["a"], vectors=True, diag_add=0.5), _sym_ref, tol=F64TOL,
    ref32=False, src="metrics_f32.hip")
_ew("row_sqrt_norm_f64[b2,n13]", "row_sqrt_norm_f64", lambda: {"B": _m64(2, 13, 13, seed=1)}, lambda ops, T: ops.row_sqrt_norm_f64(T["B"]),
    lambda R: R["B"].norm(dim=-1).sqrt(), tol=F64TOL, src="metrics_f32.hip")
_ew("transpose_f64[b2,n37]", "transpose_f64", lambda: {"a": _m64(2, 37, 37, seed=1)}, lambda ops, T: ops.transpose_f64(T["a"]), lambda R: R["a"].transpose(1, 2).contiguous(),
    tol=0, src="metrics_f32.hip")
_ew("sqrtm_vjp_div_f64[b2,n13]", "sqrtm_vjp_div_f64", lambda: {"m": _m64(2, 13, 13, seed=1), "s": _m64(2, 13, seed=2).abs() + 0.5},
    lambda ops, T: ops.sqrtm_vjp_div_f64(T["m"], T["s"]), lambda R: R["m"] / (R["s"][:, :, None] + R["s"][:, None, :]), tol=F64TOL, src="metrics_f32.hip")
_ew("to_f64[n1027]", "to_f64", lambda: {"a": rn(1027, seed=1)}, lambda ops, T: ops.to_f64(T["a"]), lambda R: R["a"].double(), tol=0, src="metrics_f32.hip")
_ew("fid_finish[d37]", "fid_finish", lambda: {"mx": rn(37, seed=1), "my": rn(37, seed=2), "cx": _m64(37, 37, seed=3), "cy": _m64(37, 37, seed=4), "sq": _m64(37, seed=5).abs()},
    lambda ops, T: ops.fid_finish(T["mx"], T["my"], T["cx"], T["cy"], T["sq"]),
    lambda R: (R["mx"] - R["my"]).pow(2).sum() + R["cx"].trace() + R["cy"].trace() - 2 * R["sq"].sum(), tol=2.0 ** -22, ref32=False, src="metrics_f32.hip")


@case("jacobi_rows[b2,n13]", "jacobi_rows", "metrics_f32.hip")
def _(ops):
    a = _m64(2, 13, 13, seed=1)
    a = a + a.transpose(1, 2)

    def call(T):
        B, Vt = ops.jacobi_rows(T["B"], T["Vt"])
        lam = B.norm(dim=-1)
        # what the solve promises: rows of B = V^T A mutually orthogonal with norms |lambda_i|, Vt = V^T orthogonal
        return lam.sort(dim=-1).values, Vt @ Vt.transpose(1, 2), Vt.transpose(1, 2) @ B

    def ref(R):
        return torch.linalg.eigvalsh(a).abs().sort(dim=-1).values, torch.eye(13, dtype=F64).expand(2, 13, 13), a
    # test_sqrtm_eig_matches_fp64's gate is at least 2e-6 on the fp32 result; the fp64 factors themselves: the rotation threshold jacobi_tol(n) ~ 6e-15 per
    # pair, accumulated over n^2 / 2 pairs and a few sweeps: 1e-11
    return dict(ins={"B": a.clone(), "Vt": torch.eye(13, dtype=F64).expand(2, 13, 13).contiguous()}, inplace=("B", "Vt"), call=call, ref=ref, tol=1e-11)


# ---- the optimizer (tests/test_training_gpu.py: _parity -- max|hip - fp64| <= 4 max|torch fp32 - fp64| per tensor) ----------------------------

SIZES = (5, 8191, 3 * 8193)
LR, BETAS, WD, DECAY, STEP1 = 1e-2, (0.9, 0.95), 1e-2, 0.37, 5.0        # parameter 1 has taken 5 steps already: a second bucket in each launch


def _opt_ins():
    ins = {}
    for i, n in enumerate(SIZES):
        ins.update({f"p{i}": rn(n, seed=10 * i + 1), f"g{i}": rn(n, seed=10 * i + 2, scale=3.0), f"m{i}": rn(n, seed=10 * i + 3, scale=0.1),
                    f"v{i}": rn(n, seed=10 * i + 4, scale=0.1).square(), f"e{i}": rn(n, seed=10 * i + 5)})
    return ins


class _Holder(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t, requires_grad=True) for t in tensors])


def _torch_step(ins, dtype):
    """Two rounds of clip_grad_norm_ + AdamW + lerp_ + zero_grad on the CPU in ``dtype`` (gradients g, then h): p, g after zero_grad, m, v, ema
    per tensor, then the two gradient norms"""
    ps = [torch.nn.Parameter(ins[f"p{i}"].to(dtype).clone()) for i in range(3)]
    opt = torch.optim.AdamW(ps, lr=LR, betas=BETAS, weight_decay=WD, foreach=False)
    for i, p in enumerate(ps):
        opt.state[p] = {"step": torch.tensor(STEP1 if i == 1 else 0.0), "exp_avg": ins[f"m{i}"].to(dtype).clone(), "exp_avg_sq": ins[f"v{i}"].to(dtype).clone()}
    emas, norms = [ins[f"e{i}"].to(dtype).clone() for i in range(3)], []
    for which in "gh":
        for i, p in enumerate(ps):
            p.grad = ins[f"{which}{i}"].to(dtype).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(ps, 1.0).detach())
        opt.step()
        for p, ema in zip(ps, emas):
            ema.lerp_(p.detach(), 1 - DECAY)
    out = []
    for p, ema in zip(ps, emas):
        out += [p.detach(), torch.zeros_like(p), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ema]
    return out + norms


@case("AdamW.step[clip,ema,zero_grad,two buckets,two steps]", "AdamW.step", "optim_f32.hip", kernel="mt_adamw_ema_f32")
def _(ops):
    import k_diffusion_amd as KD
    ins = _opt_ins()
    ins.update({f"h{i}": rn(n, seed=10 * i + 6, scale=0.02) for i, n in enumerate(SIZES)})      # second gradients: norm below the clip threshold
    f32 = _torch_step(ins, F32)

    def call(T):
        model, avg = _Holder([T[f"p{i}"] for i in range(3)]), _Holder([T[f"e{i}"] for i in range(3)])
        for i, p in enumerate(model.ps):
            assert p.data_ptr() == T[f"p{i}"].data_ptr()
            p.grad = T[f"g{i}"]
        opt = KD.optim.AdamW(model.parameters(), lr=LR, betas=BETAS, weight_decay=WD)
        for i, p in enumerate(model.ps):
            opt.state[p] = {"step": torch.tensor(STEP1 if i == 1 else 0.0), "exp_avg": T[f"m{i}"], "exp_avg_sq": T[f"v{i}"]}
        opt.attach_ema(model, avg)
        norm1 = opt.step(clip_grad_norm=1.0, ema_decay=DECAY, zero_grad=True).clone()
        table = opt._table.table.data_ptr()
        for i in range(3):                           # the second step: new gradients in the same buffers, the cached descriptor table, other bias corrections
            T[f"g{i}"].copy_(T[f"h{i}"])
        norm2 = opt.step(clip_grad_norm=1.0, ema_decay=DECAY, zero_grad=True).clone()
        assert opt._table.table.data_ptr() == table
        return [T[f"{k}{i}"] for i in range(3) for k in "pgmve"] + [norm1, norm2]

    def yardstick(j):
        def tol(got, ref):
            e_hip, e_ref = (got.detach().cpu().double() - ref).abs().max().item(), (f32[j].double() - ref).abs().max().item()
            assert e_hip <= 4 * e_ref, f"max|hip - fp64| {e_hip:.3e} > 4 x max|torch fp32 - fp64| {e_ref:.3e}"
            return e_hip
        return tol
    return dict(ins=ins, inplace=tuple(k for k in ins if k[0] != "h"), call=call, ref=lambda R: _torch_step(R, F64), tol=[yardstick(j) for j in range(17)])


@case("ema_update[5,8191,24579]", "ema_update", "optim_f32.hip")
def _(ops):
    import k_diffusion_amd as KD
    ins = {k: v for k, v in _opt_ins().items() if k[0] in "pe"}

    def call(T):
        model, avg = _Holder([T[f"p{i}"] for i in range(3)]), _Holder([T[f"e{i}"] for i in range(3)])
        KD.optim.ema_update(model, avg, DECAY)
        return [T[f"e{i}"] for i in range(3)]
    # test_training_gpu.py compares the stand-alone lerp with torch.lerp at rtol 1e-6 / atol 1e-7; in the max norm of values of order 1: 1e-6
    return dict(ins=ins, inplace=("e0", "e1", "e2"), call=call, ref=lambda R: [R[f"e{i}"].lerp(R[f"p{i}"], 1 - DECAY) for i in range(3)], tol=1e-6)


# evaluated in fp64 and rounded once to fp32: 2^-23 of the largest value (fp64 output: the libm differences of exp, 1e-13)
_ew("sigma_density[loguniform,3x37]", "sigma_density", lambda: {"u": ru(3, 37, seed=1)}, lambda ops, T: ops.sigma_density(nat.DENSITY_LOGUNIFORM, T["u"], [-3.0, 4.0]),
    lambda R: torch.exp(R["u"] * 7.0 - 3.0), tol=2.0 ** -23, ref32=False, src="optim_f32.hip")
_ew("sigma_density[loguniform,f64,stratified,3x37]", "sigma_density", lambda: {"u": ru(3, 37, seed=1).double()},
    lambda ops, T: ops.sigma_density(nat.DENSITY_LOGUNIFORM, T["u"], [-3.0, 4.0], group=1, groups=2, dtype=F64),
    lambda R: torch.exp((1 + torch.arange(37, dtype=F64) * 2 + R["u"]) / (37 * 2) * 7.0 - 3.0), tol=F64TOL, src="optim_f32.hip")


# ---- the test ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def arithmetic(request, KD, monkeypatch):
    """The case's arithmetic mode, and the few-rows kernels off unless the case asks for them (as the autouse fixture of tests/test_ops_gpu.py does)."""
    c = request.node.callspec.params["c"]
    if c.mode is not None:
        monkeypatch.setenv("KDIFF_GEMM", c.mode)
    if c.few_rows:
        yield
        return
    KD._native.set_option("x3s_max_rows", 0)
    KD._native.set_option("b16s_max_rows", 0)
    try:
        yield
    finally:
        KD._native.set_option("x3s_max_rows", -2 ** 31)
        KD._native.set_option("b16s_max_rows", -2 ** 31)


def _params():
    return [pytest.param(c, id=c.name, marks=[pytest.mark.few_rows] if c.few_rows else []) for c in CASES]


@pytest.mark.parametrize("c", _params())
def test_guard_bands(ops, c, arithmetic):
    lib = nat.lib()
    lib.kd_prof_reset()
    lib.kd_prof_enable(1)
    try:
        res = run_case(c, "nan", env=ops, device=DEV)
        names = _prof_names()
    finally:
        lib.kd_prof_enable(0)
        lib.kd_prof_reset()
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}; launches {sorted(set(names))}")
    if c.kernel is not None:
        names = [n.replace(", ", ",") for n in names]
        assert any(n.startswith(c.kernel) for n in names), f"{c.name}: expected a launch of {c.kernel}*, the profile has {sorted(set(names))}"

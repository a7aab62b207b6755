#!/usr/bin/env python3
"""KID and FID at the reference's evaluation size: 50 000 vs 50 000 feature rows of width 2048 (Inception pool3), the reference's 10 partitions
of 5 000 rows.  The HIP path (evaluation.kid: one fused Gram -> cube -> sum launch and one fixed-order reduction per partition) against a
torch restatement of k_diffusion/evaluation.py:93-123 on the same GPU (rocBLAS fp32 GEMMs, TF32 off), which is a baseline only.

    python benchmarks/metrics_bench.py [--rows 50000] [--d 2048] [--iters 3]

FID: the same features through evaluation.fid (fp64 covariances and one-sided Jacobi) against torch.cov + torch.linalg.eigh (rocSOLVER) in
fp32, with the sweep count of each of its two eigensolves and the time of one sweep at this width.

Prints one JSON line per KDIFF_GEMM mode asked for (KID) and one for FID: times from HIP events around each call after a warm-up call, the MMD kernel's
effective TFLOP/s (the 2 m n d multiply-adds of the three Gram matrices the reference computes, whether or not the kernel skips the
mirrored tiles), and the two results.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import k_diffusion_amd as K  # noqa: E402


def ev_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


def kid_torch(x, y, max_size=5000):
    """The reference's formulas on rocBLAS (evaluation.py:93-123)."""
    def kernel(a, b):
        return (a @ b.T / a.shape[-1] + 1) ** 3
    parts = K.evaluation._kid_partitions(x.shape[0], y.shape[0], max_size)
    total = x.new_zeros([])
    for (a, b), (c, d) in parts:
        cx, cy = x[a:b], y[c:d]
        m, n = cx.shape[0], cy.shape[0]
        kxx, kyy, kxy = kernel(cx, cx), kernel(cy, cy), kernel(cx, cy)
        total = total + ((kxx.sum() - kxx.diagonal().sum()) / m / (m - 1) + (kyy.sum() - kyy.diagonal().sum()) / n / (n - 1)
                         - kxy.sum() * 2 / m / n)
    return total / len(parts)


def fid_torch(x, y, eps=1e-8):
    """The reference's formulas on rocBLAS / rocSOLVER (evaluation.py:126-161)."""
    def sqrtm(a):
        vals, vecs = torch.linalg.eigh(a)
        return vecs @ vals.abs().sqrt().diag_embed() @ vecs.T
    cx, cy = torch.cov(x.T), torch.cov(y.T)
    eye = torch.eye(cx.shape[0], device=x.device, dtype=x.dtype) * eps
    cx, cy = cx + eye, cy + eye
    sx = sqrtm(cx)
    return (x.mean(0) - y.mean(0)).pow(2).sum() + torch.trace(cx + cy - 2 * sqrtm(sx @ cy @ sx))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=["split3", "exact"])
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.relu(torch.randn(args.rows, args.d, device="cuda", generator=g) + 0.2)
    y = torch.relu(torch.randn(args.rows, args.d, device="cuda", generator=g) + 0.25)
    parts = K.evaluation._kid_partitions(args.rows, args.rows)
    flops = sum(2.0 * args.d * ((b - a) ** 2 + (q - p) ** 2 + (b - a) * (q - p)) for (a, b), (p, q) in parts)
    t_ref, ref = ev_ms(lambda: kid_torch(x, y), args.iters)
    ref64 = kid_torch(x.double(), y.double()).item() if args.rows * args.d <= 50000 * 2048 else float("nan")
    for mode in args.modes:
        os.environ["KDIFF_GEMM"] = mode
        t, got = ev_ms(lambda: K.evaluation.kid(x, y), args.iters)
        print(json.dumps({"metric": "kid", "mode": mode, "rows": args.rows, "d": args.d, "partitions": len(parts), "hip_ms": round(t, 3),
                          "mmd_tflops": round(flops / t / 1e9, 1), "torch_ms": round(t_ref, 3), "speedup": round(t_ref / t, 2),
                          "hip": got.item(), "torch_fp32": ref.item(), "fp64": ref64}), flush=True)

    t_fid_ref, fid_ref = ev_ms(lambda: fid_torch(x, y), 1)
    sweeps = []

    def fid():
        out = K.evaluation.fid(x, y)
        sweeps.append(K.ops.jacobi_stats["sweeps"])        # the second solve's (S cov_y S); the first one's is not kept
        return out
    t_fid, got = ev_ms(fid, 1)
    a = torch.randn(args.d, args.d, device="cuda", generator=g)
    B, Vt = K.ops.sym_lower_f64(a[None], vectors=True)
    conv = torch.empty(args.d, device="cuda", dtype=torch.float64)
    off = torch.empty(1, device="cuda", dtype=torch.float64)

    def one_sweep():                       # one sweep with vectors on a fresh random symmetric matrix (every pair rotates)
        K.ops.nat.check(K.ops.nat.lib().kd_jacobi_sweep_f64(K.ops._p(B), K.ops._p(Vt), 1, args.d, K.ops.jacobi_tol(args.d), K.ops._p(conv),
                                                            K.ops._p(off), K.ops._stream()), "kd_jacobi_sweep_f64")
    t_sweep, _ = ev_ms(one_sweep, 1)
    print(json.dumps({"metric": "fid", "rows": args.rows, "d": args.d, "hip_ms": round(t_fid, 1), "torch_ms": round(t_fid_ref, 1),
                      "speedup": round(t_fid_ref / t_fid, 2), "sweeps_last_solve": sweeps[-1], "one_sweep_with_vectors_ms": round(t_sweep, 2),
                      "hip": got.item(), "torch_fp32": fid_ref.item(),
                      "fp64": fid_torch(x.double(), y.double()).item()}), flush=True)


if __name__ == "__main__":
    main()


"""Batch/gather driver of the sampling path and the sample-quality metrics (k_diffusion/evaluation.py:80-161).

``compute_features`` draws and gathers the samples; ``polynomial_kernel``, ``squared_mmd``, ``kid``, ``sqrtm_eig`` and ``fid`` score the
feature matrices it returns, on HIP kernels (csrc/metrics_f32.hip).  The feature extractors themselves (CLIP / Inception / DINOv2:
downloaded weights) stay out of scope: bring your own ``extractor_fn``.
"""
import math

import torch
from tqdm.auto import trange

from . import ops


def compute_features(accelerator, sample_fn, extractor_fn, n, batch_size):
    """Every rank draws ceil(n / world) samples in batches, each batch is all-gathered (RCCL over xGMI
    when ``accelerator`` is a multi-GPU ``RankContext`` / ``Accelerator``), result cut to ``n``.
    Keeps the reference's batch-size rule ``min(n - i, batch_size)`` (global ``n``, :85)."""
    per_rank = math.ceil(n / accelerator.num_processes)
    gathered = []
    try:
        for i in trange(0, per_rank, batch_size, disable=not accelerator.is_main_process):
            cur = min(n - i, batch_size)
            samples = sample_fn(cur)[:cur]
            gathered.append(accelerator.gather(extractor_fn(samples)))
    except StopIteration:
        pass
    return torch.cat(gathered)[:n]


def indexed_rounds(n, world, batch_size):
    """The gather rounds of ``compute_features_indexed``: a list of ``(width, [(lo_r, count_r) for every rank r])`` -- in a round rank r
    draws the ``count_r`` images ``lo_r .. lo_r + count_r - 1`` of its contiguous shard (``distributed.shard_range``), padded to the
    common ``width``.  A pure function of (n, world, batch_size): every rank computes every rank's share on the host, so no index
    vector has to travel with the images."""
    from .distributed import shard_range
    per = math.ceil(n / world)
    spans = [shard_range(n, world, r) for r in range(world)]
    rounds = []
    for start in range(0, per, batch_size):
        width = min(batch_size, per - start)                       # the same on every rank
        rounds.append((width, [(lo + start, max(0, min(width, hi - lo - start))) for lo, hi in spans]))
    return rounds


def compute_features_indexed(accelerator, sample_fn, n, batch_size, post=None, on_schedule=None):
    """``n`` samples addressed by GLOBAL index, independent of the process count: rank r owns the contiguous shard
    ``distributed.shard_range(n, world, r)`` and draws it in batches of at most ``batch_size``; ``sample_fn(indices)`` (a 1-D
    int64 CPU tensor, possibly empty) returns the samples of exactly those indices; every round is all-gathered (RCCL over xGMI)
    and copied into the result at the positions the HOST knows (``indexed_rounds``), so ``out[i]`` IS sample ``i`` whatever the
    batch size and the number of GPUs -- and no round waits for the device (the reference's loop, evaluation.py:84-88, does not
    either; a mask-indexed scatter would put a device->host sync behind every batch and leave the GPU idle while the next batch
    is prepared).  (``compute_features`` above keeps the reference's schedule, which sizes a rank's batches by the GLOBAL
    remainder -- evaluation.py:85 -- and returns the ranks' batches interleaved: fine for FID features, wrong for "image i of a
    seeded run".)  ``post``: applied to a rank's batch before the gather (e.g. ``ops.to_uint8``: 4x fewer bytes over xGMI).
    ``on_schedule``: called once, before the first round, with this rank's list of index tensors (one per round, in order) -- a
    sample_fn that prepares inputs ahead of time (``synth.NoisePrefetcher``) learns the whole job from it."""
    world, rank = accelerator.num_processes, accelerator.process_index
    rounds = indexed_rounds(n, world, batch_size)
    mine = [torch.arange(shares[rank][0], shares[rank][0] + shares[rank][1]) for _, shares in rounds]
    if on_schedule is not None:
        on_schedule(mine)
    out = None
    for k in trange(len(rounds), disable=not accelerator.is_main_process):
        width, shares = rounds[k]
        x = sample_fn(mine[k])
        x = x if post is None else post(x)
        if world > 1 and len(mine[k]) != width:                   # a short or empty shard: pad to the common width for the gather
            buf = x.new_zeros((width, *x.shape[1:]))
            buf[:len(mine[k])] = x
            x = buf
        g_x = accelerator.gather(x)
        if out is None:
            out = g_x.new_zeros((n, *g_x.shape[1:]))
        for r, (lo, count) in enumerate(shares):
            if count:
                out[lo:lo + count] = g_x[r * width:r * width + count]
    if out is None:                  # n == 0: no round ran and nothing tells the sample shape (the reference's torch.cat of no batches raises here)
        out = torch.empty(0, device=accelerator.device)
    return out


# ---- metrics (k_diffusion/evaluation.py:93-161).  Inputs: fp32 tensors on a ROCm device (a CPU tensor raises, as everywhere in this package).
# Only sqrtm_eig differentiates, as in the reference; kid / fid / squared_mmd / polynomial_kernel refuse a graph.

def _metric_input(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a tensor on a ROCm device (got {t.device}); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    return t.contiguous()


def _no_grad(fn, *ts):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts):
        raise NotImplementedError(f"{fn}: gradients through the metric are not implemented (only sqrtm_eig differentiates); "
                                  "call it on detached features or under torch.no_grad()")


def _feature_pair(fn, x, y):
    _no_grad(fn, x, y)
    x, y = _metric_input(x, "x"), _metric_input(y, "y")
    if x.dim() < 2 or y.dim() < 2:
        raise ValueError(f"{fn}: expected [..., rows, features] tensors, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[-1] != y.shape[-1]:
        raise ValueError(f"{fn}: x has {x.shape[-1]} features, y has {y.shape[-1]}")
    batch = torch.broadcast_shapes(x.shape[:-2], y.shape[:-2])
    x = x.expand(*batch, *x.shape[-2:]).contiguous()
    y = y.expand(*batch, *y.shape[-2:]).contiguous()
    return x, y, batch


def polynomial_kernel(x, y):
    """(x y^T / d + 1)^3 over the last two dimensions (leading dimensions broadcast), on the HIP Gram kernel."""
    x, y, _ = _feature_pair("polynomial_kernel", x, y)
    return ops.poly_kernel(x, y)


def squared_mmd(x, y, kernel=polynomial_kernel):
    """The unbiased squared MMD of rows x [..., m, d] and y [..., n, d].  With the polynomial kernel the kernel matrices are never written
    (kd_mmd_poly_f32); any other ``kernel`` callable is called for kxx, kyy, kxy and its matrices are reduced on HIP."""
    if kernel is polynomial_kernel:
        x, y, batch = _feature_pair("squared_mmd", x, y)
        return ops.mmd_poly(x, y).reshape(batch)
    _no_grad("squared_mmd", x, y)
    mats = [kernel(x, x), kernel(y, y), kernel(x, y)]
    _no_grad("squared_mmd", *mats)
    mats = [_metric_input(k, name) for k, name in zip(mats, ("kxx", "kyy", "kxy"))]
    batch = torch.broadcast_shapes(*(k.shape[:-2] for k in mats))
    kxx, kyy, kxy = (k.expand(*batch, *k.shape[-2:]).contiguous() for k in mats)
    return ops.mmd_mats(kxx, kyy, kxy).reshape(batch)


def _kid_partitions(x_size, y_size, max_size=5000):
    """The reference's partition rule (evaluation.py:118-123): [((x_lo, x_hi), (y_lo, y_hi))] per partition."""
    n_partitions = math.ceil(max(x_size / max_size, y_size / max_size))
    return [((round(i * x_size / n_partitions), round((i + 1) * x_size / n_partitions)),
             (round(i * y_size / n_partitions), round((i + 1) * y_size / n_partitions))) for i in range(n_partitions)]


def kid(x, y, max_size=5000):
    """Kernel Inception Distance: the mean squared polynomial-kernel MMD over the reference's row partitions, each partition one fused
    launch accumulating into the 0-dim result (no host sync)."""
    _no_grad("kid", x, y)
    x, y = _metric_input(x, "x"), _metric_input(y, "y")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise ValueError(f"kid: expected [rows, features] tensors of one width, got {tuple(x.shape)} and {tuple(y.shape)}")
    parts = _kid_partitions(x.shape[0], y.shape[0], max_size)
    if not parts:                  # no rows: the reference's zero over zero partitions
        return torch.full((), math.nan, device=x.device, dtype=torch.float32)
    out = torch.empty((), device=x.device, dtype=torch.float32)
    for i, ((x0, x1), (y0, y1)) in enumerate(parts):
        ops.mmd_poly(x[x0:x1], y[y0:y1], out=out, scale=1.0 / len(parts), accumulate=i > 0)
    return out


class _MatrixSquareRootEig(torch.autograd.Function):
    """V diag(sqrt|lambda|) V^T from one-sided Jacobi in fp64 (ops.jacobi_rows); backward: V (V^T g V / (d_i + d_j)) V^T, d = sqrt|lambda|
    (evaluation.py:126-140).  The products run on kd_gemm_tn_f64; the result and the gradient are rounded to fp32 once."""

    @staticmethod
    def forward(ctx, a):
        n = a.shape[-1]
        B, Vt = ops.sym_lower_f64(a.reshape(-1, n, n), vectors=True)
        ops.jacobi_rows(B, Vt)
        s = ops.row_sqrt_norm_f64(B)
        del B
        ctx.save_for_backward(Vt, s)
        return ops.gemm_tn_f64(Vt, Vt, row_scale=s, out32=True).view(a.shape)

    @staticmethod
    def backward(ctx, grad_output):
        Vt, s = ctx.saved_tensors
        n = Vt.shape[-1]
        g = ops.to_f64(_metric_input(grad_output, "grad_output").reshape(-1, n, n))
        V = ops.transpose_f64(Vt)
        m1t = ops.gemm_tn_f64(V, ops.gemm_tn_f64(g, V))                    # V^T g^T V = (V^T g V)^T
        m2t = ops.sqrtm_vjp_div_f64(m1t, s)                                # the denominator is symmetric: (M / D)^T
        return ops.gemm_tn_f64(Vt, ops.gemm_tn_f64(m2t, Vt), out32=True).view(grad_output.shape)     # V (M / D) V^T


def sqrtm_eig(a):
    """The symmetric square root V diag(sqrt|lambda|) V^T of the matrices a [..., n, n] (their lower triangles, as torch.linalg.eigh reads
    them), on a hand-written one-sided Jacobi eigensolver; differentiable with the reference's rule."""
    if a.ndim < 2:
        raise RuntimeError('tensor of matrices must have at least 2 dimensions')
    if a.shape[-2] != a.shape[-1]:
        raise RuntimeError('tensor must be batches of square matrices')
    a = _metric_input(a, "a")
    if a.numel() == 0:
        return a.new_empty(a.shape)
    return _MatrixSquareRootEig.apply(a)


def fid(x, y, eps=1e-8):
    """Frechet distance of the Gaussians fitted to the rows of x and y (evaluation.py:150-161): column means (kd_colsum_f32), centred
    covariances with divisor rows - 1 plus eps I, S = sqrtm(cov_x) on the Jacobi eigensolver, and the trace of sqrtm(S cov_y S) from the
    singular values of a second solve (no vectors).  Covariances, products and solves are fp64 from the fp32 features on; the only host reads
    are the once-per-sweep convergence tests."""
    _no_grad("fid", x, y)
    x, y = _metric_input(x, "x"), _metric_input(y, "y")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1] or x.shape[1] == 0:
        raise ValueError(f"fid: expected [rows, features] tensors of one width, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[0] < 2 or y.shape[0] < 2:
        raise ValueError(f"fid: {x.shape[0]} and {y.shape[0]} rows: a covariance needs at least 2 of each")
    covs, means = [], []
    for t in (x, y):
        tc, mean = ops.center(t)
        scale = torch.full((1, t.shape[0]), 1.0 / (t.shape[0] - 1), device=t.device, dtype=torch.float64)
        cov = ops.gemm_tn_f64(tc[None], tc[None], row_scale=scale)         # torch.cov: divisor rows - 1
        del tc
        covs.append(cov)
        means.append(mean)
    cx = ops.sym_lower_f64(covs[0], diag_add=eps)[0]
    cy = ops.sym_lower_f64(covs[1], diag_add=eps)[0]
    bx, vtx = ops.sym_lower_f64(covs[0], vectors=True, diag_add=eps)
    del covs
    ops.jacobi_rows(bx, vtx)
    sx = ops.gemm_tn_f64(vtx, vtx, row_scale=ops.row_sqrt_norm_f64(bx))   # S = sqrtm(cov_x + eps I)
    del bx, vtx
    q = ops.gemm_tn_f64(sx, ops.gemm_tn_f64(cy, sx))                      # S cov_y S (S, cov_y symmetric)
    ops.jacobi_rows(q)
    return ops.fid_finish(means[0], means[1], cx[0], cy[0], ops.row_sqrt_norm_f64(q)[0])

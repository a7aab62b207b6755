"""CPU: the metrics' public surface (evaluation.polynomial_kernel / squared_mmd / kid / sqrtm_eig / fid) against tests/golden/metrics.json, which
make_golden_metrics.py recorded from the reference (k_diffusion/evaluation.py:93-161): signatures, an fp64 restatement of the recorded
values, the partition rule and the CPU refusals.  The HIP results are checked in test_metrics_gpu.py."""
import inspect
import json
import math

import pytest
import torch

from tests.golden import make_golden_metrics as gm


@pytest.fixture(scope="module")
def gold():
    with open(gm.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ev():
    import k_diffusion_amd
    return k_diffusion_amd.evaluation


@pytest.mark.parametrize("name", ["polynomial_kernel", "squared_mmd", "kid", "sqrtm_eig", "fid"])
def test_signatures_match_the_reference(ev, gold, name):
    assert gm.signature(getattr(ev, name)) == gold["signatures"][name]
    assert inspect.signature(ev.squared_mmd).parameters["kernel"].default is ev.polynomial_kernel


def _mmd64(x, y):
    d = x.shape[1]
    kxx, kyy, kxy = ((a @ b.T / d + 1) ** 3 for a, b in ((x, x), (y, y), (x, y)))
    m, n = x.shape[0], y.shape[0]
    return ((kxx.sum() - kxx.diagonal().sum()) / m / (m - 1) + (kyy.sum() - kyy.diagonal().sum()) / n / (n - 1) - kxy.sum() * 2 / m / n).item()


@pytest.mark.parametrize("name", [n for n, c in gm.CASES.items() if c["cpu"]])
def test_fp64_restatement_matches_the_golden(ev, gold, name):
    c = gold["cases"][name]
    x, y = gm.case_inputs(name)
    assert gm.checksum(x) == pytest.approx(c["checksum_x"], rel=1e-12) and gm.checksum(y) == pytest.approx(c["checksum_y"], rel=1e-12)
    x, y = x.double(), y.double()
    parts = ev._kid_partitions(x.shape[0], y.shape[0], c["max_size"])
    kid = sum(_mmd64(x[a:b], y[p:q]) for (a, b), (p, q) in parts) / len(parts)
    assert abs(kid - c["kid64"]) <= 1e-10 * max(1.0, abs(c["kid64"]))
    if "fid64" in c:
        cx, cy = torch.cov(x.T) + 1e-8 * torch.eye(x.shape[1], dtype=torch.float64), torch.cov(y.T) + 1e-8 * torch.eye(x.shape[1], dtype=torch.float64)

        def sqrtm(a):
            vals, vecs = torch.linalg.eigh(a)
            return vecs @ vals.abs().sqrt().diag_embed() @ vecs.T
        sx = sqrtm(cx)
        fid = ((x.mean(0) - y.mean(0)).pow(2).sum() + torch.trace(cx + cy - 2 * sqrtm(sx @ cy @ sx))).item()
        assert abs(fid - c["fid64"]) <= 1e-10 * max(1.0, abs(c["fid64"]))


@pytest.mark.parametrize("sizes", [(10000, 10000, 5000), (6000, 5000, 5000), (2500, 2100, 1000), (5001, 7, 5000), (3, 3, 5000),
                                   (7, 15001, 5000), (12345, 6789, 1000)])
def test_kid_partitions_follow_the_reference_rule(ev, sizes):
    xs, ys, max_size = sizes
    n = math.ceil(max(xs / max_size, ys / max_size))
    want = [((round(i * xs / n), round((i + 1) * xs / n)), (round(i * ys / n), round((i + 1) * ys / n))) for i in range(n)]
    got = ev._kid_partitions(xs, ys, max_size)
    assert got == want
    assert got[0][0][0] == 0 and got[-1][0][1] == xs and got[-1][1][1] == ys
    assert all(a[1] == b[0] for a, b in zip([p[0] for p in got], [p[0] for p in got][1:]))


def test_cpu_tensors_are_refused(ev):
    x = torch.rand(10, 8)
    for fn in (ev.kid, ev.fid, ev.squared_mmd, ev.polynomial_kernel):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.sqrtm_eig(x[:8])
    with pytest.raises(TypeError):
        ev.kid(x.numpy(), x)


def test_sqrtm_eig_shape_errors_are_the_references(ev):
    with pytest.raises(RuntimeError, match="tensor of matrices must have at least 2 dimensions"):
        ev.sqrtm_eig(torch.rand(4))
    with pytest.raises(RuntimeError, match="tensor must be batches of square matrices"):
        ev.sqrtm_eig(torch.rand(2, 3, 4))

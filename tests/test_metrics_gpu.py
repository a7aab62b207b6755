"""GPU: the sample-quality metrics (evaluation.kid / fid / squared_mmd / polynomial_kernel / sqrtm_eig on csrc/metrics_f32.hip) against
the reference's results recorded in tests/golden/metrics.json and against fp64 restatements of k_diffusion/evaluation.py:93-161."""
import json
import os

import pytest
import torch

from tests.golden import make_golden_metrics as gm

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    with open(gm.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K():
    import k_diffusion_amd
    return k_diffusion_amd


def _inputs(gold, name):
    x, y = gm.case_inputs(name)
    c = gold["cases"][name]
    assert gm.checksum(x) == pytest.approx(c["checksum_x"], rel=1e-12) and gm.checksum(y) == pytest.approx(c["checksum_y"], rel=1e-12)
    return x.to(DEV), y.to(DEV)


def _mmd64(x, y, kernel=None):
    """squared_mmd in fp64 (evaluation.py:100-113) and its term_1 + term_2."""
    x, y = x.double(), y.double()
    kernel = kernel or (lambda a, b: (a @ b.transpose(-2, -1) / a.shape[-1] + 1) ** 3)
    m, n = x.shape[-2], y.shape[-2]
    kxx, kyy, kxy = kernel(x, x), kernel(y, y), kernel(x, y)
    t1 = (kxx.sum([-1, -2]) - kxx.diagonal(dim1=-1, dim2=-2).sum(-1)) / m / (m - 1)
    t2 = (kyy.sum([-1, -2]) - kyy.diagonal(dim1=-1, dim2=-2).sum(-1)) / n / (n - 1)
    return t1 + t2 - kxy.sum([-1, -2]) * 2 / m / n, t1 + t2


def _kid64(x, y, max_size=5000):
    from k_diffusion_amd.evaluation import _kid_partitions
    parts = _kid_partitions(x.shape[0], y.shape[0], max_size)
    return sum(_mmd64(x[a:b], y[c:d])[0] for (a, b), (c, d) in parts) / len(parts)


def _sqrtm64(a):
    vals, vecs = torch.linalg.eigh(a.double())
    return vecs @ vals.abs().sqrt().diag_embed() @ vecs.transpose(-2, -1)


def _fid64(x, y, eps=1e-8):
    x, y = x.double(), y.double()
    cx, cy = torch.cov(x.T), torch.cov(y.T)
    eye = torch.eye(cx.shape[0], device=x.device, dtype=torch.float64) * eps
    cx, cy = cx + eye, cy + eye
    sx = _sqrtm64(cx)
    return (x.mean(0) - y.mean(0)).pow(2).sum() + torch.trace(cx + cy - 2 * _sqrtm64(sx @ cy @ sx)), torch.trace(cx + cy)


def _with_mode(mode, fn):
    old = os.environ.get("KDIFF_GEMM")
    os.environ["KDIFF_GEMM"] = mode
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["KDIFF_GEMM"]
        else:
            os.environ["KDIFF_GEMM"] = old


KID_CASES = [n for n, c in gm.CASES.items() if "kid" in c["metrics"]]
FID_CASES = [n for n, c in gm.CASES.items() if "fid" in c["metrics"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", KID_CASES)
def test_kid_matches_the_reference(K, gold, name):
    c = gold["cases"][name]
    x, y = _inputs(gold, name)
    got = K.evaluation.kid(x, y, max_size=c["max_size"])
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    err = abs(got.item() - c["kid64"])
    tol = max(4 * abs(c["kid32"] - c["kid64"]), 3e-7 * c["kid_terms"])
    assert err <= tol, (name, got.item(), c["kid64"], err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FID_CASES)
def test_fid_matches_the_reference(K, gold, name):
    c = gold["cases"][name]
    x, y = _inputs(gold, name)
    got = K.evaluation.fid(x, y)
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    err = abs(got.item() - c["fid64"])
    tol = max(4 * abs(c["fid32"] - c["fid64"]), 1e-6 * c["fid_traces"])
    print(f"fid {name}: {got.item():.6f} vs fp64 {c['fid64']:.6f} (err {err:.3e}, tol {tol:.3e}, sweeps {K.ops.jacobi_stats['sweeps']})")
    assert err <= tol, (name, got.item(), c["fid64"], err, tol)


@pytest.mark.gpu
def test_kid_of_empty_and_short_inputs_is_the_references_nan(K):
    e = torch.empty(0, 16, device=DEV)
    assert K.evaluation.kid(e, e).isnan().item()
    x = torch.rand(1, 16, device=DEV)
    assert not K.evaluation.squared_mmd(x, torch.rand(5, 16, device=DEV)).isfinite().item()     # 0 / 0 over m (m - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 37, 64, 768, 1024, 2048])
@pytest.mark.parametrize("m,n", [(67, 130), (200, 129), (64, 64)])
def test_squared_mmd_odd_sizes(K, d, m, n):
    g = torch.Generator().manual_seed(d * 1000 + m + n)
    x = torch.rand(m, d, generator=g).to(DEV)
    y = (torch.rand(n, d, generator=g) + 0.05).to(DEV)
    ref, terms = _mmd64(x, y)
    got = K.evaluation.squared_mmd(x, y)
    assert got.dim() == 0
    assert abs(got.item() - ref.item()) <= 3e-7 * terms.item(), (got.item(), ref.item())
    same = K.evaluation.squared_mmd(x, x)                          # x identical to y
    ref_same, terms_same = _mmd64(x, x)
    assert abs(same.item() - ref_same.item()) <= 3e-7 * terms_same.item(), (same.item(), ref_same.item())


@pytest.mark.gpu
def test_squared_mmd_batched_and_custom_kernel(K):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 90, 48, generator=g).to(DEV)
    y = torch.rand(1, 70, 48, generator=g).to(DEV)                # broadcast over the leading dimension
    ref, terms = _mmd64(x, y.expand(3, -1, -1))
    got = K.evaluation.squared_mmd(x, y)
    assert got.shape == (3,)
    assert ((got.double() - ref).abs() <= 3e-7 * terms).all(), (got, ref)

    def rbf(a, b):
        return torch.exp(-torch.cdist(a, b) ** 2 / a.shape[-1])
    ref_rbf, terms_rbf = _mmd64(x, y.expand(3, -1, -1), rbf)
    got_rbf = K.evaluation.squared_mmd(x, y, kernel=rbf)
    assert got_rbf.shape == (3,)
    assert ((got_rbf.double() - ref_rbf).abs() <= 1e-5 * terms_rbf).all(), (got_rbf, ref_rbf)


@pytest.mark.gpu
def test_polynomial_kernel_matrix(K):
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 100, 37, generator=g).to(DEV)
    y = torch.rand(130, 37, generator=g).to(DEV)
    got = K.evaluation.polynomial_kernel(x, y)
    ref = (x.double() @ y.double().T / 37 + 1) ** 3
    assert got.shape == (2, 100, 130)
    assert ((got.double() - ref).abs() <= 3e-5 * ref.abs()).all()          # one entry: split3's ~2^-17 per product, cubed
    exact = _with_mode("exact", lambda: K.evaluation.polynomial_kernel(x, y))
    assert ((exact.double() - ref).abs() <= 2e-6 * ref.abs()).all()


def _matrix(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    if kind == "spd":
        lam = torch.rand(n, generator=g, dtype=torch.float64) * 10 + 0.1
    elif kind == "psd_rank_deficient":
        lam = torch.rand(n, generator=g, dtype=torch.float64) * 10
        lam[n // 2:] = 0
    elif kind == "indefinite":
        lam = torch.randn(n, generator=g, dtype=torch.float64) * 5
    else:                                                          # repeated |lambda|, both signs
        lam = torch.tensor([3.0, -3.0, 2.0, 2.0], dtype=torch.float64).repeat(n // 4 + 1)[:n]
    a = q @ torch.diag(lam) @ q.T
    return ((a + a.T) / 2).float()


def _sqrtm_err(got, a):
    ref = _sqrtm64(a)
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _sqrtm_gate(a):
    """4x the reference's own fp32 error (torch.linalg.eigh in fp32), at least 2e-6 relative (Frobenius)."""
    a32 = a.cpu()
    vals, vecs = torch.linalg.eigh(a32)
    return max(4 * _sqrtm_err(vecs @ vals.abs().sqrt().diag_embed() @ vecs.transpose(-2, -1), a32), 2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 64, 257, 768])
@pytest.mark.parametrize("kind", ["spd", "psd_rank_deficient", "indefinite", "repeated"])
def test_sqrtm_eig_matches_fp64(K, n, kind):
    a = _matrix(kind, n, n + len(kind))
    got = K.evaluation.sqrtm_eig(a.to(DEV))
    assert got.shape == (n, n) and got.dtype == torch.float32
    err, gate = _sqrtm_err(got.cpu(), a), _sqrtm_gate(a)
    assert err <= gate, (kind, n, err, gate, K.ops.jacobi_stats)
    if kind == "spd":
        s = got.double().cpu()
        assert ((s @ s - a.double()).norm() / a.double().norm()).item() <= 1e-6


@pytest.mark.gpu
def test_sqrtm_eig_2048_and_square_of_root(K):
    a = _matrix("indefinite", 2048, 7)
    got = K.evaluation.sqrtm_eig(a.to(DEV)).double()
    err, gate = _sqrtm_err(got.cpu(), a), _sqrtm_gate(a)
    print(f"sqrtm 2048: rel err {err:.3e} (gate {gate:.3e}), {K.ops.jacobi_stats['sweeps']} sweeps")
    assert err <= gate
    vals, vecs = torch.linalg.eigh(a.double().to(DEV))
    absa = vecs @ vals.abs().diag_embed() @ vecs.T                  # S S = |A|
    assert ((got @ got - absa).norm() / absa.norm()).item() <= 1e-6


@pytest.mark.gpu
def test_sqrtm_eig_golden_and_batched(K, gold):
    c = gold["sqrtm"]
    a = gm.sym_matrix(c["seed"], c["eigenvalues"])
    assert gm.checksum(a) == pytest.approx(c["checksum"], rel=1e-12)
    got = K.evaluation.sqrtm_eig(a.to(DEV)).double().cpu()
    ref64, ref32 = torch.tensor(c["sqrtm64"], dtype=torch.float64), torch.tensor(c["sqrtm32"], dtype=torch.float64)
    assert (got - ref64).abs().max().item() <= max(4 * (ref32 - ref64).abs().max().item(), 1e-6)
    batch = torch.stack([_matrix(k, 5, i) for i, k in enumerate(["spd", "indefinite", "repeated", "psd_rank_deficient", "spd", "indefinite"])])
    batch = batch.view(2, 3, 5, 5)
    got_b = K.evaluation.sqrtm_eig(batch.to(DEV)).cpu()
    assert got_b.shape == (2, 3, 5, 5)
    for i in range(2):
        for j in range(3):
            assert _sqrtm_err(got_b[i, j], batch[i, j]) <= _sqrtm_gate(batch[i, j])
    lower = torch.tril(batch[0, 0]) + 100 * torch.triu(torch.ones(5, 5), 1)           # only the lower triangle is read
    assert torch.equal(K.evaluation.sqrtm_eig(lower.to(DEV)).cpu(), K.evaluation.sqrtm_eig(batch[0, 0].to(DEV)).cpu())


@pytest.mark.gpu
def test_sqrtm_eig_backward_follows_the_reference_rule(K):
    a = torch.stack([_matrix("spd", 40, 1), _matrix("indefinite", 40, 2)])
    g = torch.randn(2, 40, 40, generator=torch.Generator().manual_seed(3))
    ad = a.to(DEV).requires_grad_(True)
    K.evaluation.sqrtm_eig(ad).backward(g.to(DEV))
    vals, vecs = torch.linalg.eigh(a.double())
    d = vals.abs().sqrt().unsqueeze(-1).repeat_interleave(40, -1)
    vt = vecs.transpose(-2, -1)
    ref = vecs @ (vt @ g.double() @ vecs / (d + d.transpose(-2, -1))) @ vt
    err = ((ad.grad.double().cpu() - ref).norm() / ref.norm()).item()
    assert ad.grad.dtype == torch.float32 and err <= 1e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "split3", "bf16", "fp8"])
def test_every_arithmetic_mode_is_fp32_grade(K, gold, mode):
    name = "shifted_768"
    c = gold["cases"][name]
    x, y = _inputs(gold, name)
    kid = _with_mode(mode, lambda: K.evaluation.kid(x, y)).item()
    assert abs(kid - c["kid64"]) <= max(4 * abs(c["kid32"] - c["kid64"]), 3e-7 * c["kid_terms"]), (mode, kid)
    g = torch.Generator().manual_seed(10)
    u, v = torch.rand(150, 37, generator=g).to(DEV), torch.rand(97, 37, generator=g).to(DEV)
    ref, terms = _mmd64(u, v)
    got = _with_mode(mode, lambda: K.evaluation.squared_mmd(u, v)).item()
    assert abs(got - ref.item()) <= 3e-7 * terms.item(), (mode, got, ref.item())
    fid = _with_mode(mode, lambda: K.evaluation.fid(x, y)).item()
    assert abs(fid - c["fid64"]) <= max(4 * abs(c["fid32"] - c["fid64"]), 1e-6 * c["fid_traces"]), (mode, fid)
    a = _matrix("indefinite", 64, 9)
    s = _with_mode(mode, lambda: K.evaluation.sqrtm_eig(a.to(DEV))).cpu()
    assert _sqrtm_err(s, a) <= _sqrtm_gate(a)


@pytest.mark.gpu
def test_repeat_calls_are_bit_identical(K, gold):
    x, y = _inputs(gold, "shifted_768")
    a = _matrix("indefinite", 257, 4).to(DEV)

    def run():
        return [K.evaluation.kid(x, y, 1000), K.evaluation.squared_mmd(x[:300], y[:200]), K.evaluation.polynomial_kernel(x[:99], y[:70]),
                K.evaluation.fid(x[:500], y[:600]), K.evaluation.sqrtm_eig(a)]
    first, again = run(), run()
    for u, v in zip(first, again):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_refusals(K):
    x = torch.rand(10, 8, device=DEV)
    for bad in (x.double(), x.bfloat16(), x.half()):
        for fn in (K.evaluation.kid, K.evaluation.fid, K.evaluation.squared_mmd, K.evaluation.polynomial_kernel):
            with pytest.raises(TypeError):
                fn(bad, x)
        with pytest.raises(TypeError):
            K.evaluation.sqrtm_eig(bad[:8])
    y = torch.rand(12, 9, device=DEV)
    for fn in (K.evaluation.kid, K.evaluation.fid, K.evaluation.squared_mmd, K.evaluation.polynomial_kernel):
        with pytest.raises(ValueError):
            fn(x, y)
        with pytest.raises(NotImplementedError):
            fn(x.clone().requires_grad_(True), x)


@pytest.mark.gpu
def test_compute_features_then_fid_and_kid(K):
    """End to end: tiny model -> sampler -> compute_features with a fixed extractor -> fid / kid against the fp64 restatement."""
    from tests.golden import cases
    cfg = K.config.load_config(cases.raw_config("tiny_sw"))
    mc = cfg["model"]
    model = K.config.make_model(cfg).eval().requires_grad_(False)
    model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=3))
    den = K.Denoiser(model.to(DEV), mc["sigma_data"])
    sig = K.sampling.get_sigmas_karras(4, mc["sigma_min"], mc["sigma_max"], device=DEV)
    c, (h, w) = mc["input_channels"], mc["input_size"]
    n_cls = cfg.get("dataset", {}).get("num_classes", 0)
    counter = [0]

    def sample_fn(k):
        x = torch.stack([K.synth.synth_noise((c, h, w), 1, counter[0] + i, mc["sigma_max"]) for i in range(k)]).to(DEV)
        extra = {"class_cond": torch.arange(counter[0], counter[0] + k, device=DEV) % n_cls} if n_cls else {}
        counter[0] += k
        return K.sampling.sample_euler(den, x, sig, extra_args=extra, disable=True)

    proj = torch.randn(c * h * w, 96, generator=torch.Generator().manual_seed(8)).to(DEV) / (c * h * w) ** 0.5

    def extractor(x):                                              # a fixed random feature map: relu of a projection
        return torch.relu(x.flatten(1) @ proj)

    class One:
        num_processes, process_index, is_main_process, device = 1, 0, True, torch.device(DEV)

        def gather(self, t):
            return t

    with torch.no_grad():
        fakes = K.evaluation.compute_features(One(), sample_fn, extractor, 48, 16)
    reals = torch.relu(torch.randn(64, c * h * w, generator=torch.Generator().manual_seed(9)).to(DEV) * 0.5 @ proj)
    fid_ref, traces = _fid64(fakes, reals)
    fid = K.evaluation.fid(fakes, reals)
    assert fid.dim() == 0
    assert abs(fid.item() - fid_ref.item()) <= 1e-6 * traces.item(), (fid.item(), fid_ref.item())
    kid_ref = _kid64(fakes, reals)
    _, terms = _mmd64(fakes, reals)
    kid = K.evaluation.kid(fakes, reals)
    assert kid.dim() == 0
    assert abs(kid.item() - kid_ref.item()) <= 3e-7 * terms.item(), (kid.item(), kid_ref.item())

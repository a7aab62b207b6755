#!/usr/bin/env python3
"""Record tests/golden/metrics.json from the REAL reference's sample-quality metrics (k_diffusion/evaluation.py:93-161): the signatures of
``polynomial_kernel``, ``squared_mmd``, ``kid``, ``sqrtm_eig`` and ``fid``, and for every case its seeds and shapes, a checksum of its fp32
inputs and the reference's results on those inputs in fp64 and in fp32.  No feature matrix is stored: ``features`` / ``sym_matrix`` below
rebuild the inputs from their seeds on the CPU (the tests import them).

    python tests/golden/make_golden_metrics.py      # from the repo root, where the reference can be imported
"""
import inspect
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics.json")
FUNCTIONS = ("polynomial_kernel", "squared_mmd", "kid", "sqrtm_eig", "fid")
RANK = 64            # latent factors of the synthetic features: correlated columns, like a CNN's pooled features

# name -> {"x": (seed, rows, d, shift), "y": (...), "metrics": [...], "max_size": kid's partition size, "cpu": restated in fp64 by the CPU test}
CASES = {
    "shifted_768": {"x": (11, 3000, 768, 0.0), "y": (12, 2500, 768, 0.15), "metrics": ["kid", "fid"], "max_size": 5000, "cpu": True},
    "shifted_2048": {"x": (21, 6000, 2048, 0.0), "y": (22, 5000, 2048, 0.15), "metrics": ["kid", "fid"], "max_size": 5000, "cpu": False},
    "same_2048": {"x": (31, 10000, 2048, 0.0), "y": (32, 10000, 2048, 0.0), "metrics": ["kid", "fid"], "max_size": 5000, "cpu": False},
    "few_rows_768": {"x": (41, 500, 768, 0.0), "y": (42, 600, 768, 0.1), "metrics": ["kid", "fid"], "max_size": 5000, "cpu": True},
    "partitions_64": {"x": (51, 2500, 64, 0.0), "y": (52, 2100, 64, 0.05), "metrics": ["kid"], "max_size": 1000, "cpu": True},
}
# a symmetric indefinite matrix with repeated |lambda| (+-3, a double 2, -1, 0.5)
SQRTM_CASE = {"seed": 61, "eigenvalues": [3.0, -3.0, 2.0, 2.0, -1.0, 0.5]}


def features(seed, rows, d, shift=0.0):
    """Synthetic post-ReLU features [rows, d] (fp32): relu(z L + mu + shift + 0.3 e) with z [rows, RANK] and e [rows, d] standard normal,
    L [RANK, d] / sqrt(RANK) and mu [d] drawn from a generator seeded with ``d`` (shared by x and y), z and e from one seeded with ``seed``."""
    gm = torch.Generator().manual_seed(1000 + d)
    L = torch.randn(RANK, d, generator=gm, dtype=torch.float64) / math.sqrt(RANK)
    mu = 0.2 * torch.randn(d, generator=gm, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, RANK, generator=g, dtype=torch.float64)
    e = torch.randn(rows, d, generator=g, dtype=torch.float64)
    return torch.relu(z @ L + mu + shift + 0.3 * e).float()


def sym_matrix(seed, eigenvalues):
    """Q diag(eigenvalues) Q^T (fp32) with Q the orthogonal factor of a seeded Gaussian matrix."""
    g = torch.Generator().manual_seed(seed)
    n = len(eigenvalues)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    a = q @ torch.diag(torch.tensor(eigenvalues, dtype=torch.float64)) @ q.T
    return ((a + a.T) / 2).float()


def signature(fn):
    """inspect.signature as text, a callable default shown by its name (its repr carries an address)."""
    params = [p.replace(default=_Named(p.default.__name__)) if p.default is not p.empty and callable(p.default) else p for p in inspect.signature(fn).parameters.values()]
    return str(inspect.Signature(params))


class _Named:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


def checksum(t):
    t = t.double()
    return [float(t.sum()), float((t * t).sum())]


def case_inputs(name):
    c = CASES[name]
    return features(*c["x"]), features(*c["y"])


def mmd_terms64(x, y):
    """(term_1 + term_2) of squared_mmd in fp64: the size of the two large terms the metric is a difference of."""
    x, y = x.double(), y.double()
    d = x.shape[1]
    kxx = (x @ x.T / d + 1) ** 3
    kyy = (y @ y.T / d + 1) ** 3
    m, n = x.shape[0], y.shape[0]
    return float((kxx.sum() - kxx.diagonal().sum()) / m / (m - 1) + (kyy.sum() - kyy.diagonal().sum()) / n / (n - 1))


def main():
    sys.path.insert(0, REPO)
    from oracle import ref_import
    K = ref_import.load(with_natten=False)
    ev = K.evaluation
    out = {"signatures": {f: signature(getattr(ev, f)) for f in FUNCTIONS}, "rank": RANK, "cases": {}}
    torch.set_num_threads(os.cpu_count() or 1)
    for name, c in CASES.items():
        x, y = case_inputs(name)
        rec = {k: v for k, v in c.items()}
        rec["checksum_x"], rec["checksum_y"] = checksum(x), checksum(y)
        if "kid" in c["metrics"]:
            rec["kid64"] = float(ev.kid(x.double(), y.double(), max_size=c["max_size"]))
            rec["kid32"] = float(ev.kid(x, y, max_size=c["max_size"]))
            parts = math.ceil(max(x.shape[0] / c["max_size"], y.shape[0] / c["max_size"]))
            rec["kid_terms"] = sum(mmd_terms64(x[round(i * x.shape[0] / parts):round((i + 1) * x.shape[0] / parts)],
                                               y[round(i * y.shape[0] / parts):round((i + 1) * y.shape[0] / parts)]) for i in range(parts)) / parts
        if "fid" in c["metrics"]:
            rec["fid64"] = float(ev.fid(x.double(), y.double()))
            rec["fid32"] = float(ev.fid(x, y))
            rec["fid_traces"] = float(torch.trace(torch.cov(x.double().T)) + torch.trace(torch.cov(y.double().T)))
        out["cases"][name] = rec
        print(name, {k: v for k, v in rec.items() if k.startswith(("kid", "fid"))}, flush=True)
    a = sym_matrix(**SQRTM_CASE)
    out["sqrtm"] = dict(SQRTM_CASE, checksum=checksum(a), sqrtm64=ev.sqrtm_eig(a.double()).tolist(), sqrtm32=ev.sqrtm_eig(a).tolist())
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

"""log_likelihood on the host (no GPU): the public signature against the reference's, and the pure-host pieces of its dopri5 controller
(initial step, step update, dense output) on scalar ODEs with a closed form, with the vector arithmetic in plain torch here."""
import json
import math
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_matches_the_reference(KD):
    import inspect
    golden = json.load(open(os.path.join(REPO, "tests", "golden", "signatures.json")))
    ref = golden["sampling"]["log_likelihood"]["params"]
    got = []
    for p in inspect.signature(KD.likelihood.log_likelihood).parameters.values():
        d = p.default
        got.append([p.name, p.kind.name, "<required>" if d is inspect.Parameter.empty else repr(d)])
    assert got == ref


class TorchVec:
    """The solver's vector arithmetic in fp64 torch (HipVectorOps' contract)."""

    @staticmethod
    def combine(y0, ks, coeffs):
        return tuple(y + sum(c * k[n] for k, c in zip(ks, coeffs)) for n, y in enumerate(y0))

    @staticmethod
    def norm(ks, coeffs, y0, y1, atol, rtol):
        out = 0.0
        for n, y in enumerate(y0):
            err = sum(c * k[n] for k, c in zip(ks, coeffs))
            ref = y.abs() if y1 is None else torch.maximum(y.abs(), y1[n].abs())
            out = max(out, float((err / (atol + rtol * ref)).pow(2).mean().sqrt()))
        return out


def test_tableau_consistency(KD):
    L = KD.likelihood
    for alpha, beta in zip(L.ALPHA, L.BETA):
        assert abs(sum(beta) - alpha) < 1e-14
    assert abs(sum(L.C_SOL) - 1) < 1e-14 and abs(sum(L.C_ERROR)) < 1e-14 and abs(sum(L.C_MID) - 0.5) < 1e-14


def test_dense_output_coefficients(KD):
    L = KD.likelihood
    assert max(abs(g) for g in L.dense_coeffs(0.0)) == 0.0
    assert max(abs(a - b) for a, b in zip(L.dense_coeffs(1.0), L.C_SOL)) < 1e-13
    assert max(abs(a - b) for a, b in zip(L.dense_coeffs(0.5), L.C_MID)) < 1e-13
    # y' = 1 and y' = t (stage slopes k_i = 1, k_i = c_i h): the quartic reproduces theta and theta^2 / 2 exactly
    c = [0.0] + L.ALPHA
    for th in (0.1, 0.37, 0.8, 1.3):
        g = L.dense_coeffs(th)
        assert abs(sum(g) - th) < 1e-13
        assert abs(sum(gi * ci for gi, ci in zip(g, c)) - th * th / 2) < 1e-13


def test_step_size_rules(KD):
    L = KD.likelihood
    assert L.next_step(0.5, 0.0) == 5.0
    assert L.next_step(0.5, 1e-12) == 5.0                                 # growth capped at 10x
    assert L.next_step(0.5, 0.5) == pytest.approx(0.5 * 0.9 * 0.5 ** -0.2)
    assert L.next_step(0.5, 0.9) == 0.5                                   # accepted: never shrinks
    assert L.next_step(0.5, 2.0) == pytest.approx(0.5 * 0.9 * 2.0 ** -0.2)
    assert L.next_step(0.5, 1e9) == pytest.approx(0.1)                    # rejected: at most 5x smaller
    assert L.initial_h0(1e-6, 3.0) == 1e-6 and L.initial_h0(2.0, 4.0) == pytest.approx(0.005)
    assert L.initial_step(0.005, 4.0, 2.0) == pytest.approx(min(0.5, (0.01 / 4.0) ** 0.2))
    assert L.initial_step(0.005, 0.0, 0.0) == pytest.approx(5e-6)          # max(1e-6, h0 / 1000)


def _solve(KD, lam, t0, t1, rtol, atol):
    calls = []

    def f(t, y):
        calls.append(t)
        return (lam * y[0], y[0])               # y' = lam y, z' = y  (a state with a second, integrated component like (x, ll))
    y0 = (torch.tensor([1.0, -2.0], dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    y = KD.likelihood.dopri5(f, y0, t0, t1, rtol, atol, vec=TorchVec)
    return y, calls


def test_dopri5_scalar_closed_form(KD):
    lam, t0, t1 = -1.3, 0.01, 3.0
    (y, z), calls = _solve(KD, lam, t0, t1, 1e-7, 1e-7)
    e = math.exp(lam * (t1 - t0))
    y0 = torch.tensor([1.0, -2.0], dtype=torch.float64)
    assert torch.allclose(y, y0 * e, rtol=1e-5, atol=0)
    assert torch.allclose(z, y0 * (e - 1) / lam, rtol=1e-5, atol=0)
    # 2 evaluations before the first step, then 6 per step (first-same-as-last); every stage time inside the step it belongs to
    assert (len(calls) - 2) % 6 == 0 and len(calls) > 8
    assert calls[0] == t0 and calls[1] > t0


def test_dopri5_initial_step_and_end_point(KD):
    L = KD.likelihood
    lam, t0, t1 = 0.7, 0.5, 2.0
    (y, _), calls = _solve(KD, lam, t0, t1, 1e-4, 1e-4)
    # Hairer's rule by hand for this problem
    y0 = torch.tensor([1.0, -2.0], dtype=torch.float64)
    sc = 1e-4 + 1e-4 * y0.abs()
    d0 = max(float((y0 / sc).pow(2).mean().sqrt()), 0.0)
    d1 = max(float((lam * y0 / sc).pow(2).mean().sqrt()), float((y0 / 1e-4).pow(2).mean().sqrt()))
    h0 = L.initial_h0(d0, d1)
    assert calls[1] == pytest.approx(t0 + h0, rel=1e-12)
    d2 = max(float((lam * lam * y0 / sc).pow(2).mean().sqrt()), float((lam * y0 / 1e-4).pow(2).mean().sqrt()))
    dt = L.initial_step(h0, d1, d2)
    assert calls[2] == pytest.approx(t0 + dt / 5, rel=1e-12)               # first step: f(t0) reused, stage 1 at t0 + h / 5
    assert torch.allclose(y, y0 * math.exp(lam * (t1 - t0)), rtol=2e-4, atol=0)
    # the integration overshoots t1 and the dense output lands on it: the last stage time is past t1
    assert calls[-1] >= t1

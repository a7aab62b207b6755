"""Log likelihood of data under a denoiser (k_diffusion/sampling.py:280-301, ``log_likelihood``): the exact value from the probability-flow
ODE, not a variational bound, in nats per sample (divide by ``x[0].numel() * log 2`` for bits per dimension).

    ll, info = log_likelihood(model, x, sigma_min, sigma_max, extra_args=None, atol=1e-4, rtol=1e-4)      # info = {'fevals': n}

The state (x, ll) runs from sigma_min to sigma_max under dx/dsigma = d = (x - D(x)) / sigma and dll/dsigma = v . J_d v, one Rademacher
probe ``v = randint_like(x, 2) * 2 - 1`` drawn like the reference (same global RNG stream); the result is log N(x(sigma_max); 0,
sigma_max^2) + ll(sigma_max).

Divergence term.  The reference takes v . (v^T J) with autograd through the model.  The HIP path takes v^T (J v) forward instead: one
dual pass ``forward_jvp(x, sigma, v)`` per evaluation (``layers.Denoiser.forward_jvp``; models/jvp.py for the hourglass transformer,
``models.image_v1.ImageDenoiserModelV1.forward_jvp`` for the U-Net), then kd_ll_div_f32.  A model
without ``forward_jvp`` that is NOT an object of this package -- a user's own differentiable torch callable -- runs the reference's
autograd formulation verbatim; an object of this package without a JVP rule (the ``external`` wrappers, ``sampling.make_cfg_model_fn``)
raises NotImplementedError.  Either way the solver's vector arithmetic is HIP (kd_rk_combine_f32 / kd_rk_error_f32): ROCm tensors only.

The integrator is dopri5 as torchdiffeq runs it (restated here; torchdiffeq is not a dependency, and step-for-step identity with it is
not pinned by a test -- DESIGN.md section 8):
  - Dormand-Prince 5(4) tableau, first-same-as-last: 6 new evaluations per step, accepted or rejected;
  - f0 = f(sigma_min), then the initial step by Hairer's rule at order 4: scale = atol + rtol |y0|, d0 = ||y0 / scale||,
    d1 = ||f0 / scale||, h0 = 0.01 d0 / d1 (1e-6 if d0 or d1 < 1e-5), f1 = f(sigma_min + h0, y0 + h0 f0), d2 = ||(f1 - f0) / scale|| / h0,
    h1 = (0.01 / max(d1, d2))^(1/5) (max(1e-6, h0 / 1000) if both <= 1e-15), h = min(100 h0, h1): 2 evaluations before the first step;
  - error ratio = mixed norm over (x, ll): the largest of each tensor's RMS, over the whole batch, of err / (atol + rtol max(|y0|, |y1|));
  - a step is accepted if the ratio <= 1; the next step is h min(10, max(0.9 ratio^(-1/5), dfactor)) with dfactor = 1 if ratio < 1
    else 0.2, and 10 h when the ratio is 0;
  - steps run until sigma >= sigma_max, then the quartic dense output of the last accepted step (Shampine's dopri5 midpoint
    coefficients) is evaluated at sigma_max.
Host scalars are float64; one host read per step (both error sums at once).
"""
import math

import torch

from . import ops

__all__ = ["log_likelihood"]

# Dormand-Prince 5(4)
ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
C_SOL = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
C_ERROR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400,
           11 / 84 - 649 / 6300, -1. / 60.]
C_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2, 187940372067 / 1594534317056 / 2,
         -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]
ORDER = 5
SAFETY, IFACTOR, DFACTOR = 0.9, 10.0, 0.2
MAX_STEPS = 1 << 20


# ---- pure-host pieces of the controller ----------------------------------------------------------------------------------------

def initial_h0(d0, d1):
    """First probe step of Hairer's rule from d0 = ||y0 / scale|| and d1 = ||f0 / scale||."""
    return 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1


def initial_step(h0, d1, d2, order=ORDER - 1):
    """Hairer's initial step from the probe h0, d1 and d2 = ||(f(t0 + h0) - f0) / scale|| / h0."""
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1. / float(order + 1))
    return min(100 * h0, h1)


def next_step(h, ratio, order=ORDER):
    """Step size after a step of size h with error ratio ``ratio`` (accepted or not)."""
    if ratio == 0:
        return h * IFACTOR
    dfactor = 1.0 if ratio < 1 else DFACTOR
    return h * min(IFACTOR, max(SAFETY / ratio ** (1. / order), dfactor))


def dense_coeffs(theta):
    """gamma[0..6] such that the dopri5 dense output at t0 + theta h is y0 + h sum_i gamma_i k_i (k_0 = f(t0), k_6 = f(t0 + h)): the
    quartic through y0, y1 = y0 + h C_SOL.k, y_mid = y0 + h C_MID.k with end slopes k_0, k_6 (torchdiffeq's _interp_fit /
    _interp_evaluate, expanded; the y0 terms of its coefficients cancel)."""
    e0 = [1., 0, 0, 0, 0, 0, 0]
    e6 = [0, 0, 0, 0, 0, 0, 1.]
    a = [2 * (e6[i] - e0[i]) - 8 * C_SOL[i] + 16 * C_MID[i] for i in range(7)]
    b = [5 * e0[i] - 3 * e6[i] + 14 * C_SOL[i] - 32 * C_MID[i] for i in range(7)]
    c = [e6[i] - 4 * e0[i] - 5 * C_SOL[i] + 16 * C_MID[i] for i in range(7)]
    return [theta * e0[i] + theta ** 2 * c[i] + theta ** 3 * b[i] + theta ** 4 * a[i] for i in range(7)]


class HipVectorOps:
    """The solver's vector arithmetic on tuples of ROCm fp32 tensors (kd_rk_combine_f32, kd_rk_error_f32)."""

    @staticmethod
    def combine(y0, ks, coeffs):
        """y0 + sum_j coeffs[j] ks[j] per component (terms with a zero coefficient are not read)."""
        out = []
        for n, y in enumerate(y0):
            terms = [(k[n], c) for k, c in zip(ks, coeffs) if c != 0]
            out.append(ops.rk_combine(y, [t for t, _ in terms], [c for _, c in terms]) if terms else y.clone())
        return tuple(out)

    @staticmethod
    def norm(ks, coeffs, y0, y1, atol, rtol):
        """Mixed norm: max over components of RMS(sum_j coeffs[j] ks[j] / (atol + rtol max(|y0|, |y1|))); one host read."""
        parts = []
        for n, y in enumerate(y0):
            terms = [(k[n], c) for k, c in zip(ks, coeffs) if c != 0]
            parts.append(ops.rk_error_partial([t for t, _ in terms], [c for _, c in terms], y, None if y1 is None else y1[n], atol, rtol))
        sums = torch.stack([p.double().sum() for p in parts]).tolist()
        return max(math.sqrt(s / y.numel()) for s, y in zip(sums, y0))


def dopri5(func, y0, t0, t1, rtol, atol, vec=HipVectorOps):
    """y(t1) of dy/dt = func(t, y) from y(t0) = y0 (a tuple of tensors), t1 > t0, by the rules of the module docstring.  ``vec`` supplies
    ``combine`` and ``norm`` (HipVectorOps on the device)."""
    t0, t1 = float(t0), float(t1)
    f0 = func(t0, y0)
    d0 = vec.norm([y0], [1.], y0, None, atol, rtol)
    d1 = vec.norm([f0], [1.], y0, None, atol, rtol)
    h0 = initial_h0(d0, d1)
    f1 = func(t0 + h0, vec.combine(y0, [f0], [h0]))
    d2 = vec.norm([f1, f0], [1., -1.], y0, None, atol, rtol) / h0
    dt = initial_step(h0, d1, d2)
    t, y, f, last = t0, y0, f0, None
    steps = 0
    while t1 > t:
        if not (dt > 0 and math.isfinite(dt)):
            raise RuntimeError(f"dopri5: step size {dt} at t = {t} (non-finite derivative?)")
        if steps >= MAX_STEPS:
            raise RuntimeError(f"dopri5: more than {MAX_STEPS} steps")
        steps += 1
        k = [f]
        yi = y
        for alpha, beta in zip(ALPHA, BETA):
            yi = vec.combine(y, k, [b * dt for b in beta])
            k.append(func(t + dt if alpha == 1. else t + alpha * dt, yi))
        ratio = vec.norm(k, [c * dt for c in C_ERROR], y, yi, atol, rtol)
        if ratio <= 1:
            last = (t, dt, y, k)
            t, y, f = t + dt, yi, k[-1]
        dt = next_step(dt, ratio)
    if last is None:
        return y
    ts, hs, ys, ks = last
    gamma = dense_coeffs((t1 - ts) / hs)
    return vec.combine(ys, ks, [g * hs for g in gamma])


# ---- the public function --------------------------------------------------------------------------------------------------------

def _package_object(model):
    pkg = __name__.rpartition(".")[0]
    mod = getattr(model, "__module__", None) or type(model).__module__
    return isinstance(mod, str) and (mod == pkg or mod.startswith(pkg + "."))


def log_likelihood(model, x, sigma_min, sigma_max, extra_args=None, atol=1e-4, rtol=1e-4):
    """(ll [B], {'fevals': n}): log likelihood of ``x`` under the denoiser ``model`` (see the module docstring)."""
    extra_args = {} if extra_args is None else extra_args
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"log_likelihood: the HIP path needs x on a ROCm device (got {getattr(x, 'device', type(x))}); there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"log_likelihood: fp32 inputs only (got {x.dtype})")
    rule = getattr(model, "forward_jvp", None)
    if rule is None and _package_object(model):
        name = getattr(model, "__qualname__", type(model).__name__)
        raise NotImplementedError(f"log_likelihood: {name} has no forward_jvp rule (no forward-mode JVP rule for this wrapper); "
                                  f"wrap a native model in layers.Denoiser, or give the model a forward_jvp(x, sigma, x_dot, **kwargs)")
    x = x.contiguous()
    B = x.shape[0]
    s_in = x.new_ones([B])
    v = torch.randint_like(x, 2) * 2 - 1
    fevals = 0

    if rule is not None:
        def ode_fn(sigma, state):
            nonlocal fevals
            xs = state[0]
            sig = torch.full((B,), sigma, device=x.device, dtype=torch.float32)
            denoised, denoised_dot = rule(xs, sig, v, **extra_args)
            fevals += 1
            return ops.ll_div(xs, denoised.contiguous(), denoised_dot.contiguous(), v, sig)
    else:
        def ode_fn(sigma, state):               # the reference's formulation (sampling.py:286-294), for a differentiable torch model
            nonlocal fevals
            sigma = x.new_tensor(sigma)
            with torch.enable_grad():
                xs = state[0].detach().requires_grad_()
                denoised = model(xs, sigma * s_in, **extra_args)
                d = (xs - denoised) / sigma
                fevals += 1
                grad = torch.autograd.grad((d * v).sum(), xs)[0]
                d_ll = (v * grad).flatten(1).sum(1)
            return d.detach().contiguous(), d_ll.detach().to(torch.float32).contiguous()

    with torch.no_grad():
        y0 = (x, x.new_zeros([B]))
        latent, delta_ll = dopri5(ode_fn, y0, sigma_min, sigma_max, rtol, atol)
        ll = ops.gauss_logp(latent.contiguous(), sigma_max, add=delta_ll.contiguous())
    return ll, {'fevals': fevals}

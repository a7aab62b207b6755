#!/usr/bin/env python3
"""Record tests/golden/ll_odefn.safetensors from the REAL reference's ``log_likelihood`` (k_diffusion/sampling.py:280-301).

    python tests/golden/make_golden_ll.py            # from the repo root, where the reference can be imported

torchdiffeq is absent, so ``k_diffusion.sampling.odeint`` is replaced by a recorder: it evaluates the reference's own ODE closure -- the
denoiser under autograd, ``to_d`` and the divergence term v . (v^T J) -- at fixed (sigma, x) points and returns a dummy solution.  The
probe v comes from the reference's own ``randint_like`` draw on a seeded CPU generator and is stored beside (d, d_ll).  The
neighbourhood case runs the reference's block on the oracle's restated na2d (NATTEN is absent), as every golden here.
"""
import os
import sys

import torch
from safetensors.torch import save_file

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import ref_import  # noqa: E402
from tests.golden import cases  # noqa: E402

# (config, batch); every case is evaluated at each of LL_SIGMAS, x = unit noise * sqrt(sigma^2 + sigma_data^2)
LL_CASES = [("tiny_global", 2), ("tiny_sw", 2), ("tiny_na", 2)]
LL_SIGMAS = [0.3, 4.0]
LL_SEED = 1234


def ll_points(cfg, batch, seed=21):
    """The recorded points' x (one per sigma in LL_SIGMAS) and the class ids of a case."""
    m = cfg["model"]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(batch, m["input_channels"], *m["input_size"], generator=g)
    xs = [z * (s ** 2 + m["sigma_data"] ** 2) ** 0.5 for s in LL_SIGMAS]
    nc = cases.num_classes_of(cfg)
    cls = (torch.arange(batch) * 7 + 2) % (nc + 1) if nc else None
    return xs, cls


def main():
    K = ref_import.load(with_natten=True)
    out = {}
    for name, batch in LL_CASES:
        cfg = K.config.load_config(cases.raw_config(name))
        model = K.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(cases.synth.synth_state_dict(model.state_dict(), seed=cases.WEIGHT_SEED))
        den = K.Denoiser(model, sigma_data=cfg["model"]["sigma_data"])
        xs, cls = ll_points(cfg, batch)
        extra = {"class_cond": cls} if cls is not None else {}
        rec = []

        def recorder(fn, y0, t, atol, rtol, method):
            assert method == "dopri5"
            for s, x in zip(LL_SIGMAS, xs):
                d, d_ll = fn(t.new_tensor(s), (x, y0[1]))
                rec.append((d.detach().clone(), d_ll.detach().clone()))
            return torch.stack([y0[0], y0[0]]), torch.stack([y0[1], y0[1]])

        K.sampling.odeint = recorder
        torch.manual_seed(LL_SEED)
        K.sampling.log_likelihood(den, xs[0], cfg["model"]["sigma_min"], cfg["model"]["sigma_max"], extra_args=extra)
        torch.manual_seed(LL_SEED)
        out[f"{name}.v"] = torch.randint_like(xs[0], 2) * 2 - 1
        for i, (d, d_ll) in enumerate(rec):
            out[f"{name}.{i}.d"], out[f"{name}.{i}.d_ll"] = d, d_ll
            print(f"{name} sigma={LL_SIGMAS[i]}: |d|max {d.abs().max():.4f}  d_ll {d_ll.tolist()}", flush=True)
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(cases.GOLDEN_DIR, "ll_odefn.safetensors"))


if __name__ == "__main__":
    main()

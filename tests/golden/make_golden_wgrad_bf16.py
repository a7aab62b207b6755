#!/usr/bin/env python3
"""Record tests/golden/wgrad_bf16.json: the error of the REAL reference's own bf16 training arithmetic, per parameter.

For tiny_global, tiny_sw and tiny_na at batch 2 (the weights and inputs of tests/test_param_grad_gpu.py) the reference's ``Denoiser.loss``
runs twice on the CPU: in fp64, and in fp32 under ``torch.autocast('cpu', torch.bfloat16)`` (what its train.py does under
``--mixed-precision bf16``).  ``mean(losses)`` is differentiated both times and

    err_ref[name] = max|g_bf16 - g_fp64| / max|g_fp64|

goes to the JSON ({config: {parameter name: err_ref}}): names and numbers only.  tests/test_wgrad_bf16_gpu.py holds this project's bf16
weight gradients to it.

    python tests/golden/make_golden_wgrad_bf16.py      # from the repo root, where the reference can be imported
"""
import copy
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import ref_import  # noqa: E402
from tests.golden import cases  # noqa: E402
from tests.test_param_grad_gpu import _inputs  # noqa: E402

CONFIGS = ("tiny_global", "tiny_sw", "tiny_na")
BATCH = 2


def grads_of(K, model, sigma_data, x, noise, sigma, kw, autocast):
    model.zero_grad(set_to_none=True)
    den = K.Denoiser(model, sigma_data)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        losses = den.loss(x, noise, sigma, **kw)
    losses.float().mean().backward() if autocast else losses.mean().backward()
    return {n: p.grad.detach().double() for n, p in model.named_parameters()}


def main():
    K = ref_import.load(with_natten=True)
    out = {}
    for name in CONFIGS:
        cfg = K.config.load_config(cases.raw_config(name))
        model = K.config.make_model(cfg).eval()
        model.load_state_dict(cases.synth.synth_state_dict(model.state_dict(), seed=cases.WEIGHT_SEED))
        x, noise, sigma, kw = _inputs(cfg, BATCH)
        sd = cfg["model"]["sigma_data"]
        model64 = copy.deepcopy(model).double()
        kw64 = {k: (v.double() if v.is_floating_point() else v) for k, v in kw.items()}
        g64 = grads_of(K, model64, sd, x.double(), noise.double(), sigma.double(), kw64, autocast=False)
        g16 = grads_of(K, model, sd, x, noise, sigma, kw, autocast=True)
        out[name] = {n: float((g16[n] - g64[n]).abs().max() / g64[n].abs().max()) for n in sorted(g64)}
        worst = max(out[name], key=out[name].get)
        print(f"{name}: {len(out[name])} parameters, err_ref in [{min(out[name].values()):.3e}, {out[name][worst]:.3e}] (worst: {worst})",
              flush=True)
    path = os.path.join(cases.GOLDEN_DIR, "wgrad_bf16.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/unet_wgrad_bf16.json: the error of the REAL reference's own bf16 training arithmetic on the image_v1 U-Net, per parameter.

For ``unet_a`` and ``unet_b`` of tests/unet_ref.py (``K.synth`` weights at ``unet_ref.SEED``, sigma_data 0.5, the seeded batch of
``tests/unet_train_ref.batch``) the reference's ``Denoiser.loss`` over its own ``ImageDenoiserModelV1`` (in eval mode: no dropout) runs twice on
the CPU for the weightings 'karras' and 'soft-min-snr': in fp64, and in fp32 under ``torch.autocast('cpu', torch.bfloat16)`` (what its train.py
does under ``--mixed-precision bf16``).  ``mean(losses)`` is differentiated both times and

    err_ref[name] = max|g_bf16 - g_fp64| / max|g_fp64|

goes to the JSON ({config: {weighting: {parameter name: err_ref}}}): names and numbers only.  tests/test_unet_mixed_gpu.py holds this
project's bf16 weight gradients to it.

    python tests/golden/make_golden_unet_wgrad_bf16.py      # from the repo root, where the reference can be imported
"""
import copy
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTINGS = ("karras", "soft-min-snr")


def grads_of(ref, model, weighting, sigma_data, x, noise, sigma, kw, autocast):
    model.zero_grad(set_to_none=True)
    den = ref.layers.Denoiser(model, sigma_data=sigma_data, weighting=weighting)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        losses = den.loss(x, noise, sigma, **kw)
    losses.float().mean().backward() if autocast else losses.mean().backward()
    return {n: p.grad.detach().double() for n, p in model.named_parameters()}


def main():
    sys.path.insert(0, REPO)
    import k_diffusion_amd as K
    from oracle import ref_import
    from tests import unet_ref
    from tests import unet_train_ref as tr
    ref = ref_import.load()
    out = {}
    for name, raw in unet_ref.CONFIGS.items():
        cfg = ref.config.load_config(raw)
        model = ref.config.make_model(cfg).eval()
        model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=unet_ref.SEED))
        model64 = copy.deepcopy(model).double()
        x, noise, sigma, aug = tr.batch(name)
        kw = {} if aug is None else {"aug_cond": aug}
        kw64 = {k: v.double() for k, v in kw.items()}
        out[name] = {}
        for weighting in WEIGHTINGS:
            g64 = grads_of(ref, model64, weighting, tr.SIGMA_DATA, x.double(), noise.double(), sigma.double(), kw64, autocast=False)
            g16 = grads_of(ref, model, weighting, tr.SIGMA_DATA, x.float(), noise.float(), sigma.float(), kw, autocast=True)
            err = {n: float((g16[n] - g64[n]).abs().max() / g64[n].abs().max()) for n in sorted(g64)}
            out[name][weighting] = err
            worst = max(err, key=err.get)
            print(f"{name} {weighting}: {len(err)} parameters, err_ref in [{min(err.values()):.3e}, {err[worst]:.3e}] (worst: {worst})", flush=True)
    path = os.path.join(HERE, "unet_wgrad_bf16.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/unet_train.json from the REAL reference on the CPU in fp64: ``Denoiser.loss`` (k_diffusion/layers.py:76-86) over the
reference's ``ImageDenoiserModelV1`` (built by its own ``config.make_model``, so with its ``KarrasAugmentWrapper`` where the config asks for one)
and ``torch.autograd`` through it.

For each tiny config of tests/unet_ref.py: ``K.synth`` weights at ``unet_ref.SEED`` (never the default init: its zero-initialised output layers
make almost every gradient vanish), sigma_data 0.5, the seeded batch of ``tests/unet_train_ref.batch``.  Recorded per weighting ('karras',
'soft-min-snr', 'snr'): the per-sample losses, and for ``losses.mean().backward()`` per parameter the gradient's L2 norm and its inner product
with the probe cos(0.37 arange(numel) + 1).  Kilobytes of numbers, not megabytes of gradients.

    python tests/golden/make_golden_unet_train.py      # from the repo root, where the reference can be imported
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))


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
        model = model.double()
        x, noise, sigma, aug = tr.batch(name)
        kw = {} if aug is None else {"aug_cond": aug.double()}
        out[name] = {}
        for weighting in tr.WEIGHTINGS:
            den = ref.layers.Denoiser(model, sigma_data=tr.SIGMA_DATA, weighting=weighting)
            model.zero_grad(set_to_none=True)
            losses = den.loss(x.double(), noise.double(), sigma.double(), **kw)
            losses.mean().backward()
            grads = {k: tr.summary(p.grad) for k, p in model.named_parameters()}
            assert all(v[0] > 0 for v in grads.values()), "a zero gradient tests nothing"
            out[name][weighting] = {"losses": losses.tolist(), "grads": grads}
            print(f"{name} {weighting}: losses {losses.tolist()}, {len(grads)} parameters, smallest |grad| {min(v[0] for v in grads.values()):.3e}")
    with open(os.path.join(HERE, "unet_train.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/unet_v1.safetensors and unet_v1.json from the REAL reference's ``ImageDenoiserModelV1`` (k_diffusion/models/image_v1.py,
built by the reference's own ``config.make_model``, so with its ``KarrasAugmentWrapper`` where the config asks for one) on the CPU in fp32.

For each tiny config of tests/unet_ref.py: the model gets ``K.synth`` weights (a function of the parameter names and a seed), runs on the seeded
inputs of ``unet_ref.inputs`` and its OUTPUT is recorded -- inputs and weights come back from the seeds.  The json holds the sorted state_dict
keys and shapes, the weight-format contract a checkpoint relies on.

    python tests/golden/make_golden_unet_v1.py      # from the repo root, where the reference can be imported
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, REPO)
    from safetensors.torch import save_file
    import k_diffusion_amd as K
    from oracle import ref_import
    from tests import unet_ref
    ref = ref_import.load()
    tensors, meta = {}, {}
    for name, raw in unet_ref.CONFIGS.items():
        cfg = ref.config.load_config(raw)
        model = ref.config.make_model(cfg).eval().requires_grad_(False)
        sd = K.synth.synth_state_dict(model.state_dict(), seed=unet_ref.SEED)
        model.load_state_dict(sd)
        x, sigma, aug = unet_ref.inputs(name)
        with torch.no_grad():
            out = model(x, sigma, aug_cond=aug) if aug is not None else model(x, sigma)
        assert out.abs().max() > 1e-3, "a zero output tests nothing"
        tensors[name + ".out"] = out.contiguous()
        meta[name] = {k: list(v.shape) for k, v in sorted(model.state_dict().items())}
        print(f"{name}: out {tuple(out.shape)} |max| {out.abs().max():.4f}, {len(meta[name])} state_dict entries")
    save_file(tensors, os.path.join(HERE, "unet_v1.safetensors"))
    with open(os.path.join(HERE, "unet_v1.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/unet_bf16.safetensors: the outputs of the REAL reference's ``ImageDenoiserModelV1`` (built by the reference's own
``config.make_model``) under ``torch.autocast('cpu', dtype=torch.bfloat16)``, on the weights and inputs of tests/golden/unet_v1.safetensors
(``K.synth`` weights of ``unet_ref.SEED``, the seeded inputs of ``unet_ref.inputs``).

The distance of these outputs from the fp32 outputs recorded in unet_v1.safetensors is the reference's OWN bf16 error on these inputs: the
envelope ``set_conv_arithmetic("bf16")`` is held to (tests/test_unet_bf16_gpu.py).  The fp32 forward is run again here and must reproduce the
recorded output, so that both files are known to describe the same model.

    python tests/golden/make_golden_unet_bf16.py      # from the repo root, where the reference can be imported
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, REPO)
    from safetensors.torch import load_file, save_file
    import k_diffusion_amd as K
    from oracle import ref_import
    from tests import unet_ref
    ref = ref_import.load()
    fp32 = load_file(os.path.join(HERE, "unet_v1.safetensors"))
    tensors = {}
    for name, raw in unet_ref.CONFIGS.items():
        cfg = ref.config.load_config(raw)
        model = ref.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=unet_ref.SEED))
        x, sigma, aug = unet_ref.inputs(name)
        kw = {} if aug is None else {"aug_cond": aug}
        with torch.no_grad():
            out32 = model(x, sigma, **kw)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = model(x, sigma, **kw)
        gold = fp32[name + ".out"]
        drift = (out32 - gold).abs().max().item()
        assert drift <= 1e-5 * gold.abs().max().item(), f"{name}: the fp32 forward is {drift:.3e} from the recorded one: not the same model"
        out = out.float().contiguous()
        err = (out - gold).abs().max().item()
        assert err > 0, "an autocast forward equal to the fp32 one measures nothing"
        tensors[name + ".out_autocast_bf16"] = out
        print(f"{name}: autocast(bf16) output {tuple(out.shape)} ({out.dtype}), max-norm error {err:.3e} against the fp32 output "
              f"(|max| {gold.abs().max():.4f})")
    save_file(tensors, os.path.join(HERE, "unet_bf16.safetensors"))


if __name__ == "__main__":
    main()

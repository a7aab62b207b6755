#!/usr/bin/env python3
"""Record tests/golden/unet_drop.json from the REAL reference on the CPU in fp64, in TRAINING mode with dropout: ``Denoiser.loss``
(k_diffusion/layers.py:76-86) over the reference's ``ImageDenoiserModelV1`` with ``dropout_rate`` 0.25 and ``torch.autograd`` through it.

The reference draws its masks inside two torch functions: ``torch.nn.functional.dropout2d`` (nn.Dropout2d, image_v1.py:22,26) and
``torch.nn.functional.scaled_dot_product_attention(dropout_p=p)`` (layers.py:196).  Both are patched here with stand-ins that take their keep
masks from this script and record them; the SDPA stand-in is spelt out as torch documents the function: softmax(q k^T / sqrt(d)), then
mask / (1 - p), then @ v.  That the stand-ins sit where torch's functions sit is asserted first: with every factor 1 the patched training-mode
run equals the UNPATCHED eval run of the same weights in a ``dropout_rate`` 0 model to <= 1e-12 (rate 0 there because the reference hands
``dropout_p`` to SDPA in eval mode too).

For each tiny config of tests/unet_ref.py: ``K.synth`` weights at ``unet_ref.SEED``, sigma_data 0.5, the seeded batch of
``tests/unet_train_ref.batch``, keep masks from ``torch.rand(...) >= 0.25`` under a seeded generator (every site has dropped and kept
elements).  Recorded: the masks in forward order as packed hex bit strings, and per weighting ('karras', 'soft-min-snr', 'snr') under those
same masks the per-sample losses and, for ``losses.mean().backward()``, per parameter the gradient's L2 norm and its inner product with the
probe cos(0.37 arange(numel) + 1).  Recorded results only.

    python tests/golden/make_golden_unet_drop.py      # from the repo root, where the reference can be imported
"""
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))


class Masks:
    """The two stand-ins and the masks they use.  mode "ones": every factor is 1; "draw": keep masks from the generator, recorded in call
    order; "replay": the recorded masks again, in the same order."""

    def __init__(self, rate, seed):
        self.rate, self.gen, self.mode, self.recorded, self.at = rate, torch.Generator().manual_seed(seed), "ones", [], 0

    def start(self, mode):
        self.mode, self.at = mode, 0
        if mode == "draw":
            self.recorded = []

    def factor(self, shape, p, like):
        assert p == self.rate, f"the reference asked for rate {p}, the config says {self.rate}"
        if self.mode == "ones":
            return torch.ones(shape, dtype=like.dtype)
        if self.mode == "draw":
            self.recorded.append(torch.rand(shape, generator=self.gen) >= p)
        keep = self.recorded[self.at]
        self.at += 1
        assert tuple(keep.shape) == tuple(shape)
        return keep.to(like.dtype) / (1.0 - p)

    def dropout2d(self, input, p=0.5, training=True, inplace=False):
        assert training and input.dim() == 4
        return input * self.factor(input.shape[:2], p, input)[:, :, None, None]

    def sdpa(self, query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None):
        assert attn_mask is None and not is_causal and scale is None
        prob = torch.softmax(query @ key.transpose(-2, -1) / math.sqrt(query.shape[-1]), dim=-1)
        return (prob * self.factor(prob.shape, dropout_p, prob)) @ value


def main():
    sys.path.insert(0, REPO)
    import k_diffusion_amd as K
    from oracle import ref_import
    from tests import unet_drop_ref as dr
    from tests import unet_ref
    from tests import unet_train_ref as tr
    ref = ref_import.load()
    F = torch.nn.functional
    real = (F.dropout2d, F.scaled_dot_product_attention)
    out = {}
    for name in unet_ref.CONFIGS:
        cfg = ref.config.load_config(dr.dropping_config(name))
        model = ref.config.make_model(cfg)
        sd = K.synth.synth_state_dict(model.state_dict(), seed=unet_ref.SEED)
        model.load_state_dict(sd)
        model = model.double().train()
        clean = ref.config.make_model(ref.config.load_config(unet_ref.CONFIGS[name]))
        clean.load_state_dict(sd)
        clean = clean.double().eval()
        x, noise, sigma, aug = tr.batch(name)
        kw = {} if aug is None else {"aug_cond": aug.double()}
        args = (x.double(), noise.double(), sigma.double())
        masks = Masks(dr.RATE, 3000 + len(name))
        den = lambda m, w: ref.layers.Denoiser(m, sigma_data=tr.SIGMA_DATA, weighting=w)
        with torch.no_grad():
            want = den(clean, "karras").loss(*args, **kw)              # unpatched, eval, rate 0
        F.dropout2d, F.scaled_dot_product_attention = masks.dropout2d, masks.sdpa
        try:
            masks.start("ones")
            with torch.no_grad():
                got = den(model, "karras").loss(*args, **kw)
            gap = ((got - want).abs() / want.abs()).max().item()
            print(f"{name}: stand-ins with every factor 1 against the unpatched eval run: {gap:.3e}")
            assert gap <= 1e-12
            out[name] = {"rate": dr.RATE}
            for weighting in tr.WEIGHTINGS:
                masks.start("draw" if weighting == tr.WEIGHTINGS[0] else "replay")
                model.zero_grad(set_to_none=True)
                losses = den(model, weighting).loss(*args, **kw)
                assert masks.at == len(masks.recorded)
                losses.mean().backward()
                grads = {k: tr.summary(p.grad) for k, p in model.named_parameters()}
                assert all(v[0] > 0 for v in grads.values()), "a zero gradient tests nothing"
                out[name][weighting] = {"losses": losses.tolist(), "grads": grads}
                print(f"{name} {weighting}: losses {losses.tolist()}, {len(grads)} parameters, {len(masks.recorded)} masks")
        finally:
            F.dropout2d, F.scaled_dot_product_attention = real
        assert all(bool(m.any()) and not bool(m.all()) for m in masks.recorded), "a site without a dropped or without a kept element"
        sites = dr.site_list(sd)
        assert len(sites) == len(masks.recorded)
        out[name]["masks"] = [dict(dr.pack(m), kind=kind, prefix=prefix) for m, (_, kind, prefix) in zip(masks.recorded, sites)]
    with open(os.path.join(HERE, "unet_drop.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

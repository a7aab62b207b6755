#!/usr/bin/env python3
"""Record tests/golden/augment.json from the REAL reference's ``KarrasAugmentationPipeline.__call__`` (k_diffusion/augmentation.py:40-89) on
the CPU: for every case the float32 3 x 3 matrix the reference handed to ``skimage.transform.AffineTransform``, its ``cond`` and the raw
parameters a0 .. a7 behind them.

scikit-image is not installed where this runs, so ``skimage.transform`` is a stand-in written here: an ``AffineTransform`` that keeps the
matrix it is given and a ``warp`` that returns its input.  With these the reference module imports and composes its matrix; the
INTERPOLATION is not recorded (tests/test_augment_gpu.py checks it against a restatement of scikit-image's rule).  The raw parameters are
recovered by replaying the reference's torch draws in its order under the same seed; the replay is asserted to reproduce the recorded cond
bit for bit.

    python tests/golden/make_golden_augment.py      # from the repo root, where the reference can be imported
"""
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment.json")
SIZES = [(16, 16), (20, 12)]                                     # PIL (width, height)
SEEDS = [(seed, 1.0) for seed in range(16)] + [(seed, 0.12) for seed in (100, 101, 102, 103, 104, 105)]


class AffineTransform:
    """Keeps the matrix: the stand-in for skimage.transform.AffineTransform."""
    recorded = []

    def __init__(self, matrix=None):
        self.params = np.array(matrix)
        AffineTransform.recorded.append(self.params.copy())

    @property
    def inverse(self):
        return self


def warp(image, inverse_map, **kwargs):
    assert kwargs["order"] == 3 and kwargs["mode"] == "reflect"  # the rule the device kernel restates
    return image


def replay(seed, a_prob):
    """a0 .. a7 under ``seed``, from torch draws in the reference's order (augmentation.py:44-70): a bit; then per group its gate followed by
    its values -- (bit), (normal), (angle), (angle, normal), (normal, normal)."""
    torch.manual_seed(seed)

    def bit():
        return torch.randint(2, []).float()

    def gate():
        return (torch.rand([]) < a_prob).float()

    def angle():
        return torch.rand([]) * 2 * math.pi - math.pi
    out = [bit()]
    for group in ([bit], [torch.randn], [angle], [angle, torch.randn], [torch.randn, torch.randn]):
        do = gate()
        out += [(draw([]) if draw is torch.randn else draw()) * do for draw in group]
    return torch.stack(out)


def main():
    from PIL import Image
    sys.path.insert(0, REPO)
    from oracle import ref_import
    K = ref_import.load(with_natten=False)
    stand_in = sys.modules["skimage.transform"]
    stand_in.AffineTransform, stand_in.warp = AffineTransform, warp
    assert K.augmentation.transform is stand_in
    cases = []
    for width, height in SIZES:
        image = Image.fromarray(np.zeros((height, width, 3), dtype=np.uint8), mode="RGB")
        assert image.size == (width, height)
        for seed, a_prob in SEEDS:
            pipe = K.augmentation.KarrasAugmentationPipeline(a_prob=a_prob)
            AffineTransform.recorded.clear()
            torch.manual_seed(seed)
            out, orig, cond = pipe(image)
            assert tuple(out.shape) == (3, height, width) and len(AffineTransform.recorded) == 1
            mat = AffineTransform.recorded[0]
            assert mat.dtype == np.float32 and mat.shape == (3, 3)
            raw = replay(seed, a_prob)
            a = raw
            again = torch.stack([a[0], a[1], a[2], a[3].cos() - 1, a[3].sin(), a[5] * a[4].cos(), a[5] * a[4].sin(), a[6], a[7]])
            assert torch.equal(again, cond), (seed, a_prob, again, cond)
            cases.append({"seed": seed, "a_prob": a_prob, "width": width, "height": height, "matrix": [[float(v) for v in row] for row in mat],
                          "cond": [float(v) for v in cond], "raw": [float(v) for v in raw]})
    out = {"a_scale": pipe.a_scale, "a_aniso": pipe.a_aniso, "a_trans": pipe.a_trans, "cases": cases}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    fired = sum(any(v != 0 for v in c["raw"][1:]) for c in cases)
    print(f"{len(cases)} cases ({fired} with a gate fired) -> {GOLDEN}")


if __name__ == "__main__":
    main()

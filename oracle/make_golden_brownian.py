#!/usr/bin/env python3
"""Records one query of the reference's OWN BrownianTreeNoiseSampler / BatchedBrownianTree (k_diffusion/sampling.py:65-114) with
``torchsde.BrownianTree`` replaced by oracle.brownian.OracleBrownianTree -- the stand-in make_golden_r3.py installs -- into
tests/golden/brownian_sampler.safetensors, so that tests/test_host_cpu.py::test_oracle_brownian_tree_stands_in_for_torchsde checks the
reference's sign / scaling / batching of the tree wherever the suite runs.
Run in the build container (the reference is imported through oracle/ref_import's stubs):  python oracle/make_golden_brownian.py"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import brownian as ob  # noqa: E402
from oracle import ref_import  # noqa: E402

# the query of the test: batch of 2 (seeds 7, 8), 3 x 8 x 8 images, tree over [0.01, 160], descending sigmas 4 -> 1
SEEDS, SHAPE, SIGMA_MIN, SIGMA_MAX, SIGMA, SIGMA_NEXT = [7, 8], (2, 3, 8, 8), 0.01, 160.0, 4.0, 1.0


def main():
    R = ref_import.load()
    R.sampling.torchsde.BrownianTree = ob.OracleBrownianTree
    ns = R.sampling.BrownianTreeNoiseSampler(torch.zeros(SHAPE), SIGMA_MIN, SIGMA_MAX, seed=SEEDS)
    noise = ns(torch.tensor(SIGMA), torch.tensor(SIGMA_NEXT)).contiguous()
    from safetensors.torch import save_file
    path = os.path.join(REPO, "tests", "golden", "brownian_sampler.safetensors")
    save_file({"noise": noise}, path, metadata={"seeds": str(SEEDS), "sigma_min": str(SIGMA_MIN), "sigma_max": str(SIGMA_MAX),
                                                "sigma": str(SIGMA), "sigma_next": str(SIGMA_NEXT), "torch": torch.__version__})
    print(path, tuple(noise.shape))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the device augmentation of a training batch: ``kd_augment_draw_f32`` + ``kd_augment_warp_f32`` (K.augmentation.augment_draw /
augment_warp) at a CIFAR batch (64 x 3 x 32^2) and at 32 x 3 x 256^2, a_prob = 1 (every sample is warped; the cost does not depend on it).

    python benchmarks/augment_bench.py [--warmup 10] [--repeats 7] [--inner 50] [--out profiles/augment_bench.jsonl]

HIP events around ``inner`` back-to-back draw + warp pairs (host launch cost included, as a training loop pays it) after ``warmup`` pairs;
``repeats`` such samples, the median and the min / max reported.  Bytes: the batch read once and written once (8 per element; the 16-tap
gather hits cache); the achieved rate is that over the median time, set against the 4.6 TB/s a streaming copy reaches on this chip
("HBM").  A record, not a gate.  Prints one JSON line per shape and appends it to ``--out`` if given.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import k_diffusion_amd as K  # noqa: E402

SHAPES = [(64, 3, 32, 32), (32, 3, 256, 256)]
COPY_TBS = 4.6              # streaming copy on the MI355X as DESIGN.md records it


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("augment_bench.py needs a ROCm device")
    aug = K.augmentation
    for shape in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(0)
        x = torch.rand(shape, device="cuda", generator=gen) * 2 - 1
        key = torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device="cuda", generator=gen)
        raw, y = torch.empty(shape[0], 8, device="cuda"), torch.empty_like(x)

        def pair():
            aug.augment_draw(key, shape[0], 1.0, out=raw)
            aug.augment_warp(x, raw, out=y)

        def warp_only():
            aug.augment_warp(x, raw, out=y)
        out = {"bench": "augment", "shape": list(shape), "bytes": 8 * x.numel()}
        for name, fn in (("draw_warp", pair), ("warp", warp_only)):
            for _ in range(args.warmup):
                fn()
            ts = sorted(sample(fn, args.inner) for _ in range(args.repeats))
            med = statistics.median(ts)
            out[name] = {"median_us": round(med * 1e3, 2), "min_us": round(ts[0] * 1e3, 2), "max_us": round(ts[-1] * 1e3, 2)}
            out[name + "_tb_per_s"] = round(out["bytes"] / (med * 1e-3) / 1e12, 4)
            out[name + "_copy_fraction"] = round(out[name + "_tb_per_s"] / COPY_TBS, 4)
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()

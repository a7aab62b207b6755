#!/usr/bin/env python3
"""Cost of the dual pass behind log_likelihood (k-diffusion_amd/models/jvp.py) against one ``forward`` of the same denoiser, and the
evaluations and wall time of one ``log_likelihood`` call.  Synthetic weights (synth.py), fp32 split3 arithmetic by default.

    python benchmarks/ll_bench.py [--config configs/config_oxford_flowers.json] [--batches 1 8 32] [--ll-batch 1] [--iters 5]

Prints one JSON line per batch size ({"batch", "forward_ms", "dual_ms", "ratio"}) and one for the log_likelihood call.  Times are
host clocks around work that ends in a device synchronise, after one warm-up call of every shape.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import k_diffusion_amd as K  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(REPO, "configs", "config_oxford_flowers.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ll-batch", type=int, default=1, help="batch of the log_likelihood call (0: skip it)")
    ap.add_argument("--sigma", type=float, default=2.0)
    args = ap.parse_args()
    os.environ.setdefault("KDIFF_GEMM", "split3")
    cfg = K.config.load_config(json.load(open(args.config)))
    mc = cfg["model"]
    model = K.config.make_model(cfg).eval().requires_grad_(False)
    model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=1))
    model = model.to("cuda")
    den = K.Denoiser(model, mc["sigma_data"])
    nc = cfg.get("dataset", {}).get("num_classes", 0)
    shape = (mc["input_channels"], *mc["input_size"])
    for B in args.batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, *shape, device="cuda", generator=g) * (args.sigma ** 2 + mc["sigma_data"] ** 2) ** 0.5
        v = torch.randint(0, 2, x.shape, device="cuda", generator=g).float() * 2 - 1
        sig = torch.full((B,), args.sigma, device="cuda")
        kw = {"class_cond": torch.arange(B, device="cuda") % nc} if nc else {}
        fwd = timed(lambda: den(x, sig, **kw), args.iters)
        dual = timed(lambda: den.forward_jvp(x, sig, v, **kw), args.iters)
        print(json.dumps({"config": os.path.basename(args.config), "mode": os.environ["KDIFF_GEMM"], "batch": B, "forward_ms": round(fwd, 3),
                          "dual_ms": round(dual, 3), "ratio": round(dual / fwd, 2)}), flush=True)
    if args.ll_batch:
        B = args.ll_batch
        torch.manual_seed(0)
        x = torch.randn(B, *shape, device="cuda") * mc["sigma_data"]
        kw = {"class_cond": torch.arange(B, device="cuda") % nc} if nc else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ll, info = K.likelihood.log_likelihood(den, x, mc["sigma_min"], mc["sigma_max"], extra_args=kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        dims = x[0].numel()
        print(json.dumps({"config": os.path.basename(args.config), "log_likelihood_batch": B, "fevals": info["fevals"], "wall_s": round(wall, 2),
                          "bits_per_dim": [round(-float(l) / dims / 0.6931471805599453, 4) for l in ll.cpu()]}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of a training step's gradients (``Denoiser.loss`` + backward into every parameter, models/vjp.py) against one ``forward`` of the same
denoiser, and the peak device memory of each.  Synthetic weights (synth.py), ``eval()``, fp32 split3 arithmetic by default; with
``--dropout`` the training step runs in training mode with ``model.enable_dropout()`` at the config's rates (``--dropout-rate`` sets them);
``--wgrad bf16`` runs the weight-gradient GEMMs on bf16 operands (``model.set_wgrad_arithmetic``).

    python benchmarks/train_bench.py [--config configs/config_oxford_flowers.json] [--batches 1 8 32] [--iters 3] [--dropout] [--dropout-rate 0 0 0.1] [--wgrad bf16]

Prints one JSON line per batch size ({"batch", "forward_ms", "train_ms", "ratio", "forward_peak_mib", "train_peak_mib"}).  Times are host
clocks around work that ends in a device synchronise, after one warm-up call of every shape; the peaks are torch.cuda.max_memory_allocated
over one call after a reset, above what was allocated before it (inputs, weights and the gradients of the previous call).
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


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(REPO, "configs", "config_oxford_flowers.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=2.0)
    ap.add_argument("--dropout", action="store_true", help="train in training mode with model.enable_dropout() at the config's dropout rates "
                                                             "(the forward still runs in eval())")
    ap.add_argument("--dropout-rate", type=float, nargs="+", default=None, help="per-level dropout rates (one value: every level) in place "
                                                                                 "of the config's")
    ap.add_argument("--wgrad", choices=["bf16"], default=None, help="model.set_wgrad_arithmetic: bf16 weight-gradient GEMMs (default: the "
                                                                    "backward pass's rule)")
    args = ap.parse_args()
    os.environ.setdefault("KDIFF_GEMM", "split3")
    raw = json.load(open(args.config))
    if args.dropout_rate is not None:
        raw["model"]["dropout_rate"] = args.dropout_rate[0] if len(args.dropout_rate) == 1 else args.dropout_rate
    cfg = K.config.load_config(raw)
    mc = cfg["model"]
    model = K.config.make_model(cfg).eval()
    model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=1))
    model = model.to("cuda")
    if args.dropout:
        model.enable_dropout()
    model.set_wgrad_arithmetic(args.wgrad)
    den = K.Denoiser(model, mc["sigma_data"])
    nc = cfg.get("dataset", {}).get("num_classes", 0)
    shape = (mc["input_channels"], *mc["input_size"])
    for B in args.batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, *shape, device="cuda", generator=g) * mc["sigma_data"]
        noise = torch.randn(x.shape, device="cuda", generator=g)
        sig = torch.full((B,), args.sigma, device="cuda")
        kw = {"class_cond": torch.arange(B, device="cuda") % nc} if nc else {}

        def fwd():
            model.eval()
            with torch.no_grad():
                return den(x, sig, **kw)

        def train():
            model.train(args.dropout)
            model.zero_grad(set_to_none=False)
            den.loss(x, noise, sig, **kw).mean().backward()
        t_f, t_t = timed(fwd, args.iters), timed(train, args.iters)
        m_f, m_t = peak_mib(fwd), peak_mib(train)
        print(json.dumps({"config": os.path.basename(args.config), "mode": os.environ["KDIFF_GEMM"], "batch": B, "wgrad": args.wgrad,
                          "dropout": mc["dropout_rate"] if args.dropout else None, "forward_ms": round(t_f, 3),
                          "train_ms": round(t_t, 3), "ratio": round(t_t / t_f, 2), "forward_peak_mib": round(m_f, 1),
                          "train_peak_mib": round(m_t, 1)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the optimizer tail of a training iteration: the fused HIP step (``K.optim.AdamW.step(clip_grad_norm=1, ema_decay=d,
zero_grad=True)``: one norm launch pair + one fused launch) against the same work as torch runs it on the same parameter set --
``clip_grad_norm_(1.)`` + ``torch.optim.AdamW`` (its default foreach path) + one ``lerp_`` per parameter + ``zero_grad(set_to_none=False)``.

    python benchmarks/optim_bench.py [--config configs/config_oxford_flowers.json] [--warmup 5] [--repeats 7] [--inner 10]
                                     [--train-batches 1 8 32] [--only fused|torch] [--out profiles/optim_bench.jsonl]

Synthetic weights and gradients.  HIP events around ``inner`` back-to-back steps (host launch cost included, as a training loop pays it),
after ``warmup`` steps; ``repeats`` such samples, the median and the min / max reported.  Bytes per element of the fused step: 44 by
construction (4 the norm's gradient read; 20 read + 16 written by the update: p, g, m, v, ema in, p, m, v, ema out; 4 the gradient zero);
the achieved bandwidth is that over the median time.  ``--train-batches`` also times ``Denoiser.loss`` + backward (benchmarks/train_bench.py's
training leg) and reports the step's share of the iteration.  ``--only`` runs one side and skips the rest: for a kernel trace
(launch counts) of each side on its own.  Prints one JSON line and appends it to ``--out`` if given.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import k_diffusion_amd as K  # noqa: E402

BYTES_PER_ELEMENT = 44
HBM_PEAK_TBS = 8.0          # MI355X HBM3E peak


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    ts = sorted(sample(fn, inner) for _ in range(repeats))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(REPO, "configs", "config_oxford_flowers.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--train-batches", type=int, nargs="*", default=[])
    ap.add_argument("--only", choices=["fused", "torch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("KDIFF_GEMM", "split3")
    cfg = K.config.load_config(args.config)
    mc = cfg["model"]
    model = K.config.make_model(cfg).eval()
    model.load_state_dict(K.synth.synth_state_dict(model.state_dict(), seed=1))
    model = model.to("cuda")
    oc = cfg["optimizer"]
    kw = dict(lr=oc["lr"], betas=tuple(oc["betas"]), eps=oc["eps"], weight_decay=oc["weight_decay"])
    gen = torch.Generator(device="cuda").manual_seed(0)
    decay = 0.999

    def with_grads(m):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
        return m

    n_tensors = len(list(model.parameters()))
    n_elems = sum(p.numel() for p in model.parameters())
    out = {"bench": "optim", "config": os.path.basename(args.config), "tensors": n_tensors, "elements": n_elems,
           "bytes_per_element": BYTES_PER_ELEMENT}

    if args.only in (None, "fused"):
        m_f = with_grads(copy.deepcopy(model))
        ema_f = copy.deepcopy(model)
        opt_f = K.optim.AdamW(m_f.param_groups(oc["lr"]), **kw)
        opt_f.attach_ema(m_f, ema_f)

        def fused():
            opt_f.step(clip_grad_norm=1.0, ema_decay=decay, zero_grad=True)
        out["fused"] = measure(fused, args.warmup, args.repeats, args.inner)
        tbs = BYTES_PER_ELEMENT * n_elems / (out["fused"]["median_ms"] * 1e-3) / 1e12
        out["fused_tb_per_s"] = round(tbs, 3)
        out["fused_hbm_fraction"] = round(tbs / HBM_PEAK_TBS, 3)
        del m_f, ema_f, opt_f

    if args.only in (None, "torch"):
        m_t = with_grads(copy.deepcopy(model))
        ema_t = copy.deepcopy(model)
        opt_t = torch.optim.AdamW(m_t.param_groups(oc["lr"]), **kw)
        pairs = list(zip(m_t.parameters(), ema_t.parameters()))

        def baseline():
            torch.nn.utils.clip_grad_norm_(m_t.parameters(), 1.0)
            opt_t.step()
            with torch.no_grad():
                for p, a in pairs:
                    a.lerp_(p, 1 - decay)
            opt_t.zero_grad(set_to_none=False)
        out["torch"] = measure(baseline, args.warmup, args.repeats, args.inner)
        del m_t, ema_t, opt_t, pairs

    if "fused" in out and "torch" in out:
        out["speedup"] = round(out["torch"]["median_ms"] / out["fused"]["median_ms"], 3)

    if args.train_batches and args.only is None:
        den = K.Denoiser(model, mc["sigma_data"])
        nc = cfg.get("dataset", {}).get("num_classes", 0)
        shares = []
        for B in args.train_batches:
            x = torch.randn(B, mc["input_channels"], *mc["input_size"], device="cuda", generator=gen) * mc["sigma_data"]
            noise = torch.randn(x.shape, device="cuda", generator=gen)
            sig = torch.full((B,), 2.0, device="cuda")
            ckw = {"class_cond": torch.arange(B, device="cuda") % nc} if nc else {}

            def train():
                model.zero_grad(set_to_none=False)
                den.loss(x, noise, sig, **ckw).mean().backward()
            t = measure(train, 1, 3, 1)["median_ms"]
            shares.append({"batch": B, "loss_backward_ms": t,
                           "fused_share": round(out["fused"]["median_ms"] / (t + out["fused"]["median_ms"]), 4),
                           "torch_share": round(out["torch"]["median_ms"] / (t + out["torch"]["median_ms"]), 4)})
        out["iteration_share"] = shares

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

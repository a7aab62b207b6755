#!/usr/bin/env python3
"""Forward time of the image_v1 U-Net on the HIP kernels against the same architecture as plain torch in fp32 on the same GPU.

Two models: the CIFAR-shaped one (depths [2, 4, 4], channels [128, 256, 512], 3 x 32 x 32, batch 64) and the MNIST-shaped one (channels
[128, 128, 256], 1 x 28 x 28, batch 4), both with the augment wrapper and synthetic weights.  Per model: 10 warm-up forwards of each side, then 7
samples of each, alternating, timed with HIP events; reported as median [min, max] in ms.  Three sides: the HIP forward (``hip_ms``, the
fp32-grade split-bf16 x 3 convolutions), the HIP forward after ``set_conv_arithmetic("bf16")`` on a second model object with the same weights
(``hip_bf16_ms``), and the torch side, tests/unet_ref.py's functional forward on the device (torch's conv / group-norm / SDPA kernels, depthwise
resampling): the yardstick, not the code under test.  After the timed samples one more forward of each HIP arithmetic runs under the library's
per-launch events, and the line carries the time per kernel name.

``--profile`` instead runs 3 warm-up + 5 HIP forwards of ONE model and nothing else (``--arithmetic bf16``: in the bf16 mode), for a kernel trace
of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python benchmarks/unet_bench.py --profile cifar
``--dual`` instead times the dual (primal + tangent) pass ``forward_jvp`` of ``log_likelihood`` at batch B against the forward at batch B and
the forward at batch 2 B (the dual pass stacks the tangent behind the primal: 2 B samples in every buffer), same warm-up and sampling.
``--vjp`` instead times the reverse pass at batch B -- ``forward_vjp`` plus one ``pullback`` -- against the plain forward at batch B and against
``forward_vjp`` alone (the primal on tensors of its own), same warm-up and sampling; after the timed samples one more reverse pass runs under the
library's per-launch events, and the line carries the time per kernel name (where the reverse pass's time goes).
``--train`` instead times one training evaluation at batch B -- ``Denoiser.loss(...).mean().backward()`` with every parameter trainable --
against the plain forward at batch B and against torch autograd over tests/unet_ref.py's forward in fp32 on the same GPU (the yardstick), same
warm-up and sampling, with the time per kernel name of one more evaluation; then, per 3 x 3 convolution shape of the model's levels, the weight
gradient kernel ``kd_conv2d_wgrad_x3`` against the composition that served before it existed: nine ``ops.wgrad`` calls over nine shifted,
zero-padded copies of A (timed without and with making the copies).
``--train --dropout P`` instead times the same training evaluation of a model with ``dropout_rate`` P in training mode after
``enable_dropout()`` against the SAME model in ``eval()`` (the dropout-free objective: the baseline, measured in the same session, alternating),
same warm-up and sampling, with the time per kernel name of one more evaluation of each.
``--train --wgrad bf16`` instead times the same training evaluation with and without ``set_wgrad_arithmetic("bf16")`` on the SAME model
(alternating, 5 warm-up, 7 samples), with the time per kernel name of one more evaluation of each; then, per 3 x 3 convolution shape of the
model's levels, ``kd_conv2d_wgrad_bf16`` against ``kd_conv2d_wgrad_x3`` on the same operands (alternating, 5 warm-up, 7 samples).
Prints one JSON line per model.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODELS = {
    "cifar": ({"type": "image_v1", "input_channels": 3, "input_size": [32, 32], "mapping_out": 256, "depths": [2, 4, 4], "channels": [128, 256, 512],
               "self_attn_depths": [False, True, True], "augment_wrapper": True, "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80}, 64),
    "mnist": ({"type": "image_v1", "input_channels": 1, "input_size": [28, 28], "mapping_out": 256, "depths": [2, 4, 4], "channels": [128, 128, 256],
               "self_attn_depths": [False, False, True], "augment_wrapper": True, "sigma_data": 0.6162, "sigma_min": 1e-2, "sigma_max": 80}, 4),
}


def conv_flops(model, B, H, W):
    """2 M N K of every convolution kd_conv2d_x3 serves in one forward (3 x 3, 1 x 1 skip / qkv / out projections)."""
    import k_diffusion_amd as K
    inner = model.inner_model
    plan = inner._plan(B, H, W, torch.device("cuda", torch.cuda.current_device()))
    total = 0.0
    for call in plan.calls:
        if call.func is K.unet_ops.conv2d:
            x, w, b, h, ww = call.args[:5]
            total += 2.0 * b * h * ww * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]
    return total


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_ms():
    """The library's per-launch event times since the last reset, summed per kernel name: {name: [launches, ms]}."""
    import ctypes as C
    import k_diffusion_amd as K
    lib = K._native.lib()
    out, name, ms, fl, by = {}, C.create_string_buffer(128), C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.kd_prof_count()):
        K._native.check(lib.kd_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)), "kd_prof_get")
        ent = out.setdefault(name.value.decode().split(" ")[0], [0, 0.0])
        ent[0] += 1
        ent[1] += ms.value
    lib.kd_prof_reset()
    return {k: [n, round(t, 4)] for k, (n, t) in sorted(out.items(), key=lambda kv: -kv[1][1])}


def dropout_bench(K, name, mc, sd, x, sigma, aug, B, rate):
    """The ``--train --dropout`` line of one model."""
    dev = x.device
    cfg = K.config.load_config({"model": dict(mc, dropout_rate=rate), "dataset": {"type": "imagefolder", "num_classes": 0}})
    model = K.config.make_model(cfg)
    model.load_state_dict(sd)
    model = model.to(dev).requires_grad_(True).enable_dropout(torch.Generator(device=dev).manual_seed(7))
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    den = K.Denoiser(model, 0.5)

    def run(training):
        model.train(training)
        model.zero_grad(set_to_none=True)
        den.loss(x, noise, sigma, aug_cond=aug).mean().backward()
    sides = {"eval_train_ms": lambda: run(False), "dropout_train_ms": lambda: run(True)}
    for _ in range(5):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(7):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    line = {"model": name, "batch": B, "dropout_rate": rate, **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()}}
    line["dropout_over_eval"] = line["dropout_train_ms"][0] / line["eval_train_ms"][0]
    K._native.prof_enable(True)
    for k, fn in sides.items():
        K._native.lib().kd_prof_reset()
        fn()
        torch.cuda.synchronize()
        line[k.replace("_ms", "_kernel_ms")] = kernel_ms()
    K._native.prof_enable(False)
    print(json.dumps(line), flush=True)


def level_shapes(model, H, W):
    """(h, w, c_in, c_out) of every 3 x 3 convolution shape of the model's levels."""
    ch = model.inner_model.channels
    shapes = []
    for i, c in enumerate(ch):
        for ci in sorted({c, ch[max(0, i - 1)], 2 * c if i < len(ch) - 1 else c}):
            shapes.append((H >> i, W >> i, ci, c))
    return shapes


def wgrad_bench(K, name, model, x, sigma, aug, B, H, W):
    """The ``--train --wgrad bf16`` lines of one model."""
    dev = x.device
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    den = K.Denoiser(model, 0.5)
    model.requires_grad_(True)

    def run(arithmetic):
        model.set_wgrad_arithmetic(arithmetic)
        model.zero_grad(set_to_none=True)
        den.loss(x, noise, sigma, aug_cond=aug).mean().backward()
    sides = {"split3_train_ms": lambda: run(None), "bf16_train_ms": lambda: run("bf16")}
    for _ in range(5):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(7):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    line = {"model": name, "batch": B, **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()}}
    line["bf16_over_split3"] = line["bf16_train_ms"][0] / line["split3_train_ms"][0]
    K._native.prof_enable(True)
    for k, fn in sides.items():
        K._native.lib().kd_prof_reset()
        fn()
        torch.cuda.synchronize()
        line[k.replace("_ms", "_kernel_ms")] = kernel_ms()
    K._native.prof_enable(False)
    print(json.dumps(line), flush=True)
    model.set_wgrad_arithmetic(None).requires_grad_(False)
    with torch.no_grad():
        for h, w, ci, co in level_shapes(model, H, W):
            a, gy = torch.randn(B * h * w, ci, device=dev), torch.randn(B * h * w, co, device=dev)
            sides = {"conv2d_wgrad_x3_ms": lambda: K.unet_ops.conv2d_wgrad(gy, a, B, h, w, 3),
                     "conv2d_wgrad_bf16_ms": lambda: K.unet_ops.conv2d_wgrad(gy, a, B, h, w, 3, bf16=True)}
            for _ in range(5):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in sides}
            for _ in range(7):
                for k, fn in sides.items():
                    times[k].append(timed(fn))
            x3, b16 = (fn() for fn in sides.values())
            row = {"model": name, "shape": f"B{B} {h}x{w} {ci}->{co}", **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()},
                   "chunks": K.unet_ops.conv_wgrad_chunks(B, h, w, ci, co)[1], "rel_diff": ((b16 - x3).abs().max() / x3.abs().max()).item()}
            row["bf16_over_x3"] = row["conv2d_wgrad_bf16_ms"][0] / row["conv2d_wgrad_x3_ms"][0]
            row["tflops_bf16"] = 2.0 * B * h * w * 9 * ci * co / row["conv2d_wgrad_bf16_ms"][0] / 1e9
            print(json.dumps(row), flush=True)


def train_bench(K, ur, name, model, sd, x, sigma, aug, B, H, W):
    """The ``--train`` lines of one model."""
    from torch.nn import functional as F
    dev = x.device
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(x.shape, generator=g).to(dev)
    den = K.Denoiser(model, 0.5)
    model.requires_grad_(True)

    def hip():
        model.zero_grad(set_to_none=True)
        den.loss(x, noise, sigma, aug_cond=aug).mean().backward()

    def forward():
        with torch.no_grad():
            den.loss(x, noise, sigma, aug_cond=aug)
    leaves = {k: v.detach().to(dev, torch.float32).requires_grad_(v.is_floating_point() and "kernel" not in k and "timestep_embed" not in k)
              for k, v in sd.items()}
    prepared = {(k[len("inner_model."):] if k.startswith("inner_model.") else k): v for k, v in leaves.items()}
    prepared["__wrapped__"] = True
    params = [v for v in leaves.values() if v.requires_grad]

    def ref():
        var = sigma ** 2 + 0.25
        c_skip, c_out, c_in = (t[:, None, None, None] for t in (0.25 / var, sigma * 0.5 / var.sqrt(), 1 / var.sqrt()))
        noised = x + noise * sigma[:, None, None, None]
        f = ur.forward(prepared, noised * c_in, sigma, aug_cond=aug, dtype=torch.float32, device=dev, grouped_resample=True, prepared=True)
        loss = (f - (x - c_skip * noised) / c_out).pow(2).flatten(1).mean(1).mean()
        return torch.autograd.grad(loss, params)
    sides = {"forward_ms": forward, "train_ms": hip, "torch_fp32_autograd_ms": ref}
    for _ in range(5):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(7):
        for k, fn in sides.items():
            times[k].append(timed(fn))
    line = {"model": name, "batch": B, **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()}}
    line["train_over_forward"] = line["train_ms"][0] / line["forward_ms"][0]
    line["torch_over_train"] = line["torch_fp32_autograd_ms"][0] / line["train_ms"][0]
    hip()
    named = dict(model.named_parameters())
    want = ref()
    errs = {k: ((named[k].grad - w).abs().max() / w.abs().max()).item() for k, w in zip([k for k, v in leaves.items() if v.requires_grad], want)}
    line["worst_grad_rel_diff_vs_torch_fp32"] = max(errs.values())
    K._native.prof_enable(True)
    K._native.lib().kd_prof_reset()
    hip()
    torch.cuda.synchronize()
    line["train_kernel_ms"] = kernel_ms()
    K._native.prof_enable(False)
    print(json.dumps(line), flush=True)
    model.requires_grad_(False)
    # the weight-gradient kernel against nine ops.wgrad calls over shifted copies of A, per 3 x 3 shape of the levels
    with torch.no_grad():
        for h, w, ci, co in level_shapes(model, H, W):
            a, gy = torch.randn(B * h * w, ci, device=dev), torch.randn(B * h * w, co, device=dev)

            def shifted():
                img = F.pad(a.view(B, h, w, ci), (0, 0, 1, 1, 1, 1))
                return [img[:, ky:ky + h, kx:kx + w].reshape(-1, ci).contiguous() for ky in range(3) for kx in range(3)]
            copies = shifted()
            new = lambda: K.unet_ops.conv2d_wgrad(gy, a, B, h, w, 3)
            nine = lambda: [K.ops.wgrad(gy, c) for c in copies]
            nine_with_copies = lambda: [K.ops.wgrad(gy, c) for c in shifted()]
            sides = {"conv2d_wgrad_x3_ms": new, "nine_wgrad_ms": nine, "nine_wgrad_with_copies_ms": nine_with_copies}
            for _ in range(3):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in sides}
            for _ in range(7):
                for k, fn in sides.items():
                    times[k].append(timed(fn))
            diff = (new() - torch.stack(nine(), dim=-1).view(co, ci, 3, 3)).abs().max().item() / new().abs().max().item()
            flops = 2.0 * B * h * w * 9 * ci * co
            row = {"model": name, "shape": f"B{B} {h}x{w} {ci}->{co}", **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()},
                   "chunks": K.unet_ops.conv_wgrad_chunks(B, h, w, ci, co)[1], "rel_diff": diff}
            row["nine_over_new"] = row["nine_wgrad_ms"][0] / row["conv2d_wgrad_x3_ms"][0]
            row["tflops_fp32_equiv"] = flops / row["conv2d_wgrad_x3_ms"][0] / 1e9
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", choices=sorted(MODELS))
    ap.add_argument("--arithmetic", choices=["bf16"], default=None, help="with --profile: set_conv_arithmetic('bf16') on the profiled model")
    ap.add_argument("--models", nargs="*", default=["cifar", "mnist"])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dual", action="store_true")
    ap.add_argument("--vjp", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--dropout", type=float, default=None, metavar="P", help="with --train: dropout at rate P against eval() of the same model")
    ap.add_argument("--wgrad", choices=["bf16"], default=None, help="with --train: set_wgrad_arithmetic('bf16') against the default on the same model")
    args = ap.parse_args()
    if args.dropout is not None and not args.train:
        ap.error("--dropout goes with --train")
    if args.wgrad is not None and (not args.train or args.dropout is not None):
        ap.error("--wgrad goes with --train, without --dropout")
    import k_diffusion_amd as K
    from tests import unet_ref as ur
    ur.USE_SDPA = True
    dev = torch.device("cuda")
    for name in ([args.profile] if args.profile else args.models):
        mc, B = MODELS[name]
        cfg = K.config.load_config({"model": mc, "dataset": {"type": "imagefolder", "num_classes": 0}})
        model = K.config.make_model(cfg).eval().requires_grad_(False)
        sd = K.synth.synth_state_dict(model.state_dict(), seed=1)
        model.load_state_dict(sd)
        model = model.to(dev)
        C, (H, W) = mc["input_channels"], mc["input_size"]
        g = torch.Generator().manual_seed(3)
        sigma = torch.exp(torch.randn(B, generator=g) * 1.2 - 1.2).to(dev)
        x = (torch.randn(B, C, H, W, generator=g).to(dev) * (sigma ** 2 + 0.25).sqrt()[:, None, None, None]).contiguous()
        aug = (0.5 * torch.randn(B, 9, generator=g)).to(dev)
        hip = lambda: model(x, sigma, aug_cond=aug)
        if args.train and args.dropout is not None:
            dropout_bench(K, name, mc, sd, x, sigma, aug, B, args.dropout)
            continue
        if args.train and args.wgrad is not None:
            wgrad_bench(K, name, model, x, sigma, aug, B, H, W)
            continue
        if args.train:
            train_bench(K, ur, name, model, sd, x, sigma, aug, B, H, W)
            continue
        with torch.no_grad():
            if args.profile:
                model.set_conv_arithmetic(args.arithmetic)
                for _ in range(8):
                    hip()
                torch.cuda.synchronize()
                continue
            if args.dual:
                v = (torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1).to(dev)
                x2, sigma2, aug2 = (torch.cat([t, t]) for t in (x, sigma, aug))
                sides = {"forward_ms": hip, "forward_2b_ms": lambda: model(x2, sigma2, aug_cond=aug2),
                         "dual_ms": lambda: model.forward_jvp(x, sigma, v, aug_cond=aug)}
                for _ in range(10):
                    for fn in sides.values():
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in sides}
                for _ in range(7):
                    for k, fn in sides.items():
                        times[k].append(timed(fn))
                line = {"model": name, "batch": B, **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()},
                        "dual_launches": len(model.inner_model._plan(B, H, W, x.device, dual=True).calls) + 8}
                print(json.dumps(line), flush=True)
                continue
            if args.vjp:
                u = (torch.randint(0, 2, x.shape, generator=g).float() * 2 - 1).to(dev)
                sides = {"forward_ms": hip, "primal_ms": lambda: model.forward_vjp(x, sigma, aug_cond=aug),
                         "vjp_ms": lambda: model.forward_vjp(x, sigma, aug_cond=aug)[1](u)}
                for _ in range(10):
                    for fn in sides.values():
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in sides}
                for _ in range(7):
                    for k, fn in sides.items():
                        times[k].append(timed(fn))
                line = {"model": name, "batch": B, **{k: [statistics.median(t), min(t), max(t)] for k, t in times.items()}}
                line["vjp_over_forward"] = line["vjp_ms"][0] / line["forward_ms"][0]
                K._native.prof_enable(True)
                K._native.lib().kd_prof_reset()
                sides["vjp_ms"]()
                torch.cuda.synchronize()
                line["vjp_kernel_ms"] = kernel_ms()
                K._native.prof_enable(False)
                print(json.dumps(line), flush=True)
                continue
            sd_dev = ur.prepare(sd, torch.float32, dev)
            ref = lambda: ur.forward(sd_dev, x, sigma, aug_cond=aug, dtype=torch.float32, device=dev, grouped_resample=True, prepared=True)
            # the third side: a second model object with the same weights after set_conv_arithmetic("bf16") (a change of the setting drops the
            # plans, so the two arithmetics alternate on two objects)
            model_b = K.config.make_model(cfg).eval().requires_grad_(False)
            model_b.load_state_dict(sd)
            model_b = model_b.to(dev).set_conv_arithmetic("bf16")
            hip_b = lambda: model_b(x, sigma, aug_cond=aug)
            for _ in range(10):
                hip()
                hip_b()
                if not args.no_torch:
                    ref()
            torch.cuda.synchronize()
            t_hip, t_b16, t_ref = [], [], []
            for _ in range(7):
                t_hip.append(timed(hip))
                t_b16.append(timed(hip_b))
                if not args.no_torch:
                    t_ref.append(timed(ref))
            err = None if args.no_torch else ((hip() - ref()).abs().max() / ref().abs().max()).item()
            err_b = ((hip_b() - hip()).abs().max() / hip().abs().max()).item()
            # one more forward of each arithmetic under the library's per-launch events: where the time goes
            kernels = {}
            K._native.prof_enable(True)
            for key, fn in (("hip_kernel_ms", hip), ("hip_bf16_kernel_ms", hip_b)):
                K._native.lib().kd_prof_reset()
                fn()
                torch.cuda.synchronize()
                kernels[key] = kernel_ms()
            K._native.prof_enable(False)
        flops = conv_flops(model, B, H, W)
        line = {"model": name, "batch": B, "hip_ms": [statistics.median(t_hip), min(t_hip), max(t_hip)],
                "hip_bf16_ms": [statistics.median(t_b16), min(t_b16), max(t_b16)],
                "torch_fp32_ms": None if args.no_torch else [statistics.median(t_ref), min(t_ref), max(t_ref)],
                "hip_vs_torch_rel_diff": err, "hip_bf16_vs_hip_rel_diff": err_b, "conv_gflop_per_forward": flops / 1e9,
                "launches_per_forward": len(model.inner_model._plan(B, H, W, x.device).calls) + 6, **kernels}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/training.json from the REAL reference's training helpers (k_diffusion/utils.py, k_diffusion/config.py):

  * ``_get_closed_form_lr`` of InverseLR / ExponentialLR / ConstantLRWithWarmup, called unbound on a stand-in object (the reference's
    constructors pass ``verbose`` to a torch that no longer takes it), for last_epoch = 0 .. N;
  * ``EMAWarmup.get_value()`` sequences and state dicts;  ``ema_update_dict`` sequences;
  * ``make_sample_density``: the chosen ``rand_*`` function and its bound keywords for every reference config and one hand-written
    case per remaining density type;
  * the six sigma densities on recorded uniforms (and normals), in fp32 and fp64, with ``stratified_with_settings`` / ``torch.rand`` /
    ``torch.randn`` replaced by functions that return the recorded values: the arrays go to tests/golden/training.safetensors
    (``uniforms``, ``normals``, ``<case>.fp32``, ``<case>.fp64``), the calls that made them to the JSON.

    python tests/golden/make_golden_training.py      # from the repo root, where the reference can be imported
"""
import glob
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import ref_import  # noqa: E402
from tests.golden import cases  # noqa: E402

N_EPOCHS = 12
LR_CASES = [
    ("InverseLR", dict(inv_gamma=20000.0, power=1.0, warmup=0.99, min_lr=0.0)),          # config_oxford_flowers.json's lr_sched
    ("InverseLR", dict(inv_gamma=7.0, power=0.75, warmup=0.9, min_lr=2e-5)),
    ("ExponentialLR", dict(num_steps=10, decay=0.5, warmup=0.8, min_lr=1e-5)),
    ("ExponentialLR", dict(num_steps=1000, decay=0.5, warmup=0.0, min_lr=0.0)),
    ("ConstantLRWithWarmup", dict(warmup=0.99)),
    ("ConstantLRWithWarmup", dict(warmup=0.0)),
]
BASE_LRS = [5e-4, 1.6666666666666666e-4]
EMA_CASES = [
    dict(power=0.6667, max_value=0.9999),                                                # the configs' ema_sched
    dict(inv_gamma=3.0, power=0.75, min_value=0.2, max_value=0.9, start_at=5),
    dict(inv_gamma=1.0, power=1.0, start_at=2, last_epoch=1),
]
MODEL_BASE = dict(sigma_data=0.5, sigma_min=1e-2, sigma_max=80.0, input_size=[64, 64])
HAND_DENSITIES = [
    {"type": "lognormal", "mean": -1.2, "std": 1.2},
    {"type": "lognormal", "loc": -0.5, "scale": 1.0},
    {"type": "loglogistic"},
    {"type": "loglogistic", "loc": 0.1, "scale": 0.7, "min_value": 0.01, "max_value": 80.0},
    {"type": "loguniform"},
    {"type": "loguniform", "min_value": 0.002, "max_value": 50.0},
    {"type": "v-diffusion"},
    {"type": "cosine", "min_value": 0.01, "max_value": 100.0},
    {"type": "split-lognormal", "mean": -1.0, "std_1": 1.4, "std_2": 0.9},
    {"type": "split-lognormal", "loc": 0.3, "scale_1": 0.5, "scale_2": 2.0},
    {"type": "cosine-interpolated", "noise_d_low": 16, "noise_d_high": 48, "image_d": 96, "min_value": 0.005, "max_value": 500.0},
]
N_UNIFORMS = 2048
DENSITY_CASES = {          # name -> (reference function, keywords)
    "lognormal": ("rand_log_normal", dict(loc=-1.2, scale=1.2)),
    "loglogistic": ("rand_log_logistic", dict(loc=-0.6931471805599453, scale=0.5, min_value=0.0, max_value=float("inf"))),
    "loglogistic_truncated": ("rand_log_logistic", dict(loc=0.1, scale=0.7, min_value=0.01, max_value=80.0)),
    "loguniform": ("rand_log_uniform", dict(min_value=0.01, max_value=80.0)),
    "v_diffusion": ("rand_v_diffusion", dict(sigma_data=0.5, min_value=1e-3, max_value=1e3)),
    "cosine_interpolated": ("rand_cosine_interpolated", dict(image_d=256, noise_d_low=32, noise_d_high=256, sigma_data=0.5, min_value=1e-3,
                                                             max_value=1e3)),
    "split_lognormal": ("rand_split_log_normal", dict(loc=-1.0, scale_1=1.4, scale_2=0.9)),
}


def main():
    K = ref_import.load(with_natten=True)
    out = {"n_epochs": N_EPOCHS, "base_lrs": BASE_LRS, "lr_sched": [], "ema_warmup": [], "ema_update_dict": {}, "sample_density": [],
           "densities": {}}
    for cls, kw in LR_CASES:
        fn = getattr(K.utils, cls)._get_closed_form_lr
        out["lr_sched"].append({"cls": cls, "kwargs": kw,
                                "lrs": [fn(types.SimpleNamespace(base_lrs=BASE_LRS, last_epoch=e, **kw)) for e in range(N_EPOCHS)]})
    for kw in EMA_CASES:
        sched = K.utils.EMAWarmup(**kw)
        values = []
        for _ in range(N_EPOCHS):
            values.append(sched.get_value())
            sched.step()
        out["ema_warmup"].append({"kwargs": kw, "values": values, "state_dict": sched.state_dict()})
    updates = [{"loss": 0.8}, {"loss": 0.5, "gns": 3.0}, {"loss": 0.45}, {"gns": 2.0, "loss": 0.61}]
    decays = [0.0, 0.37, 0.5503, 0.9]
    values, seq = {}, []
    for u, d in zip(updates, decays):
        K.utils.ema_update_dict(values, dict(u), d)
        seq.append(dict(values))
    out["ema_update_dict"] = {"updates": updates, "decays": decays, "values": seq}

    def record_density(name, model_config):
        part = K.config.make_sample_density(model_config)
        out["sample_density"].append({"name": name, "model": model_config, "func": part.func.__name__, "keywords": dict(part.keywords)})

    for path in sorted(glob.glob(os.path.join(ref_import.REFERENCE_ROOT, "configs", "*.json"))):
        mc = K.config.load_config(path)["model"]
        keep = {k: mc[k] for k in ("sigma_sample_density", "sigma_data", "sigma_min", "sigma_max", "input_size")}
        record_density(os.path.basename(path), keep)
    for i, sd in enumerate(HAND_DENSITIES):
        record_density(f"hand_{i}_{sd['type']}", dict(MODEL_BASE, sigma_sample_density=sd))

    gen = torch.Generator().manual_seed(20)
    u = torch.rand(N_UNIFORMS, generator=gen)
    u[0], u[1], u[2], u[3] = 0.0, 1 - 2.0 ** -24, 2.0 ** -24, 0.5
    normal = torch.randn(N_UNIFORMS, generator=gen)
    arrays = {"uniforms": u, "normals": normal}
    real = (K.utils.stratified_with_settings, torch.rand, torch.randn)
    try:
        K.utils.stratified_with_settings = lambda shape, dtype=None, device=None: u.to(dtype)
        torch.rand = lambda shape, dtype=None, device=None: u.to(dtype)
        torch.randn = lambda shape, dtype=None, device=None: normal.to(dtype)
        for name, (fn, kw) in DENSITY_CASES.items():
            f = getattr(K.utils, fn)
            out["densities"][name] = {"func": fn, "keywords": kw}
            arrays[name + ".fp32"] = f([N_UNIFORMS], dtype=torch.float32, **kw).contiguous()
            arrays[name + ".fp64"] = f([N_UNIFORMS], dtype=torch.float64, **kw).contiguous()
    finally:
        K.utils.stratified_with_settings, torch.rand, torch.randn = real
    path = os.path.join(cases.GOLDEN_DIR, "training.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    from safetensors.torch import save_file
    save_file(arrays, os.path.join(cases.GOLDEN_DIR, "training.safetensors"))
    print("wrote", path, os.path.getsize(path), "bytes, and training.safetensors")


if __name__ == "__main__":
    main()

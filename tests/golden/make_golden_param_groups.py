#!/usr/bin/env python3
"""Record tests/golden/param_groups.json from the REAL reference's ``ImageTransformerDenoiserModelV2.param_groups``
(k_diffusion/models/image_transformer_v2.py:59-84, :708-719): the parameter names of each of the four AdamW groups and the groups'
``lr`` / ``weight_decay`` keys, for two tiny configs (stored beside the names, so the test rebuilds the same models).

    python tests/golden/make_golden_param_groups.py      # from the repo root, where the reference can be imported
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import ref_import  # noqa: E402
from tests.golden import cases  # noqa: E402

BASE_LR, MAPPING_LR_SCALE = 2e-4, 0.25


def configs():
    sw = cases.raw_config("tiny_sw")                           # class-conditional, shifted window + global
    na = cases.raw_config("tiny_na")                           # three levels, merges and splits
    na["model"]["mapping_cond_dim"] = 12
    return {"tiny_sw": sw, "tiny_na_mapping_cond": na}


def main():
    K = ref_import.load(with_natten=True)
    out = {"base_lr": BASE_LR, "mapping_lr_scale": MAPPING_LR_SCALE, "cases": {}}
    for name, raw in configs().items():
        model = K.config.make_model(K.config.load_config(raw))
        names = {id(p): n for n, p in model.named_parameters()}
        groups = model.param_groups(BASE_LR, MAPPING_LR_SCALE)
        out["cases"][name] = {"config": raw, "groups": [{"params": sorted(names[id(p)] for p in grp["params"]),
                                                         **{k: v for k, v in grp.items() if k != "params"}} for grp in groups]}
    path = os.path.join(cases.GOLDEN_DIR, "param_groups.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

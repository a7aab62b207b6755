"""Training surface on the CPU: ``param_groups`` against the reference's groups (tests/golden/param_groups.json), ``Denoiser.loss``'s
signature and the refusals that need no GPU."""
import inspect
import json
import os

import pytest
import torch

from tests.golden import cases


def _golden():
    with open(os.path.join(cases.GOLDEN_DIR, "param_groups.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["tiny_sw", "tiny_na_mapping_cond"])
def test_param_groups_match_reference(KD, name):
    gold = _golden()
    case = gold["cases"][name]
    model = KD.config.make_model(KD.config.load_config(case["config"]))
    names = {id(p): n for n, p in model.named_parameters()}
    groups = model.param_groups(gold["base_lr"], gold["mapping_lr_scale"])
    assert len(groups) == len(case["groups"]) == 4
    for got, ref in zip(groups, case["groups"]):
        assert sorted(names[id(p)] for p in got["params"]) == ref["params"]
        assert {k: v for k, v in got.items() if k != "params"} == {k: v for k, v in ref.items() if k != "params"}
    assert sum(len(g["params"]) for g in groups) == len(names)
    torch.optim.AdamW(model.param_groups(1e-4))        # the train.py call


def test_loss_signature_and_cpu_refusals(KD):
    assert str(inspect.signature(KD.Denoiser.loss)) == "(self, input, noise, sigma, **kwargs)"
    model = KD.config.make_model(KD.config.load_config(cases.raw_config("tiny_global")))
    den = KD.Denoiser(model, 0.5)
    x, n, s = torch.randn(1, 3, 16, 16), torch.randn(1, 3, 16, 16), torch.tensor([1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.loss(x, n, s)
    with pytest.raises(NotImplementedError, match=r"w.r.t. sigma.*sigma\.detach\(\)"):
        den.loss(x, n, s.requires_grad_())
    with pytest.raises(NotImplementedError, match="class_cond"):
        den.loss(x, n, torch.tensor([1.0]), class_cond=torch.ones(1, requires_grad=True))
    with pytest.raises(NotImplementedError, match="scales"):
        KD.Denoiser(model, 0.5, scales=3).loss(x, n, torch.tensor([1.0]))
    for cls in (KD.layers.DenoiserWithVariance, KD.layers.SimpleLossDenoiser):
        with pytest.raises(NotImplementedError):
            cls(model, 0.5).loss(x, n, torch.tensor([1.0]))

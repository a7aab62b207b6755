"""Dropout of the training loss on the CPU: the sites of the shipped configs (``dropout_sites``), the opt-in's checks and the refusals that
come before any device work."""
import importlib

import pytest
import torch

from tests.golden import cases

SITE = 1 << 62
REFERENCE_RATES = {"mnist": 0.05, "cifar": 0.05, "flowers_sw": [0.0, 0.0, 0.1], "flowers_na": [0.0, 0.0, 0.1]}   # the reference's configs


def _itv2(KD):
    return importlib.import_module(KD.__name__ + ".models.image_transformer_v2")


def _model(KD, name, rate=None, mapping_rate=None, mapping_depth=None):
    raw = cases.raw_config(name)
    if rate is not None:
        raw["model"]["dropout_rate"] = rate
    if mapping_rate is not None:
        raw["model"]["mapping_dropout_rate"] = mapping_rate
    if mapping_depth is not None:
        raw["model"]["mapping_depth"] = mapping_depth
    return KD.config.make_model(KD.config.load_config(raw))


@pytest.mark.parametrize("name", sorted(REFERENCE_RATES))
def test_sites_of_the_shipped_configs(KD, name):
    itv2 = _itv2(KD)
    assert itv2.dropout_sites(_model(KD, name)) == []                  # the JSON files here set no rate: nothing to drop
    model = _model(KD, name, REFERENCE_RATES[name])
    sites = itv2.dropout_sites(model)
    steps = itv2.hourglass(model)
    layers = [i for i, st in enumerate(steps) if st.kind == "layer" and model.level_specs[st.level].dropout > 0]
    assert [s for s, *_ in sites] == [SITE | (2 * i + k) for i in layers for k in (0, 1)]     # every level of these configs has attention
    assert [kind for _, _, kind, _ in sites] == ["attn", "ff"] * len(layers)
    assert all(st == steps[(s - SITE) // 2] for s, st, _, _ in sites)
    if name.startswith("flowers"):
        assert len(sites) == 8 and all(st.prefix.startswith("mid_level.") and p == 0.1 for _, st, _, p in sites)
    else:
        top = len(model.level_specs) - 1
        layer_count = sum(lv.depth * (1 if i == top else 2) for i, lv in enumerate(model.level_specs))
        assert len(sites) == 2 * layer_count and all(p == 0.05 for *_, p in sites)
        assert len(sites) == {"mnist": 16, "cifar": 16}[name]


def test_mapping_sites_and_table(KD):
    itv2 = _itv2(KD)
    model = _model(KD, "tiny_sw", rate=[0.0, 0.2], mapping_rate=0.3, mapping_depth=2)
    sites = itv2.dropout_sites(model)
    assert [t for t in sites if t[2] == "mapping"] == [(SITE | 1 << 32, 0, "mapping", 0.3), (SITE | 1 << 32 | 1, 1, "mapping", 0.3)]
    level = [st for _, st, kind, _ in sites if kind != "mapping"]
    assert len(level) == 2 and all(st.level == 1 for st in level)
    key = torch.zeros(1, dtype=torch.int64)
    table = itv2.dropout_table(model, key)
    assert len(table) == len(sites) and table[("mapping", 1)] == (key, SITE | 1 << 32 | 1, 0.3)
    assert table[(level[0].prefix, "attn")][1] == sites[0][0]
    assert itv2.dropout_table(model, None) == {}


def test_enable_dropout_checks_and_refusals(KD):
    model = _model(KD, "tiny_global", rate=0.1)
    x, sigma = torch.randn(2, 3, 16, 16), torch.ones(2)
    keys = sorted(model.state_dict())
    # not enabled, training mode, a rate > 0: the training loss refuses, naming both ways out, on one line
    with pytest.raises(NotImplementedError, match=r"dropout.*model\.eval\(\)") as e:
        model.loss_forward(x, sigma)
    assert "model.enable_dropout()" in str(e.value) and "\n" not in str(e.value)
    assert model.enable_dropout() is model
    assert sorted(model.state_dict()) == keys
    for call in (lambda: model(x, sigma), lambda: model.forward_preconditioned(x, sigma, 0.5), lambda: model.forward_jvp(x, sigma, x)):
        with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
            call()
    with pytest.raises(TypeError):
        model.enable_dropout(generator=123)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            _model(KD, "tiny_global", rate=bad).enable_dropout()
    with pytest.raises(ValueError, match="mapping dropout"):
        _model(KD, "tiny_global", mapping_rate=1.0).enable_dropout()
    # every rate 0, enabled, training mode: the other passes are not refused (they get as far as the device check)
    m0 = _model(KD, "tiny_global").enable_dropout()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m0(x, sigma)


def test_dropout_argument_checks(KD):
    assert KD.ops._dropout_args(None) is None
    assert KD.ops._dropout_args((None, SITE, 0.0)) is None             # p == 0: nothing to launch
    for bad in (1.0, -0.25):
        with pytest.raises(ValueError, match="outside"):
            KD.ops._dropout_args((None, SITE, bad))

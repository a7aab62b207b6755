"""The image_v1 U-Net without a GPU: the restatement (tests/unet_ref.py) against the reference's recorded outputs, the state_dict contract, the
constructor's refusals, the ABI table, and the three pins a U-Net change walks into (``K.layers`` gains none of the reference's U-Net names)."""
import ctypes as C
import functools
import json
import os
import re

import pytest
import torch

from tests import unet_ref as ur

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NEW_ENTRY_POINTS = {"kd_pack_conv_x3": 6, "kd_conv2d_x3": 15, "kd_groupnorm_stats_f32": 9, "kd_adagn_apply_f32": 13, "kd_down2_f32": 9,
                    "kd_up2_f32": 9, "kd_unet_in_f32": 12, "kd_unet_out_f32": 13, "kd_cond_mlp_f32": 10}
PINNED = {"AdaGN", "ConditionedModule", "ConditionedResidualBlock", "ConditionedSequential", "CrossAttention2d", "Downsample2d", "ResidualBlock",
          "SelfAttention2d", "UNet", "UnconditionedModule", "Upsample2d", "dct"}


@functools.lru_cache(maxsize=None)
def golden():
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, "unet_v1.safetensors")), json.load(open(os.path.join(GOLDEN, "unet_v1.json")))


@functools.lru_cache(maxsize=None)
def built(name):
    """(merged config, model with synth weights on the CPU, its state dict)"""
    import k_diffusion_amd as K
    cfg = K.config.load_config(ur.CONFIGS[name])
    model = K.config.make_model(cfg).eval().requires_grad_(False)
    sd = K.synth.synth_state_dict(model.state_dict(), seed=ur.SEED)
    model.load_state_dict(sd)
    return cfg, model, sd


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_restatement_matches_the_reference(name):
    """fp32 restatement against the reference's fp32 output: measured 1.03e-7 (unet_a) and 2.33e-7 (unet_b) relative to the largest output."""
    _, _, sd = built(name)
    x, sigma, aug = ur.inputs(name)
    out = ur.forward(sd, x, sigma, aug_cond=aug, dtype=torch.float32)
    err = rel(out, golden()[0][name + ".out"])
    print(f"{name}: restatement (fp32) against the golden output: {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_make_model_gives_the_reference_state_dict(KD, name):
    cfg, model, sd = built(name)
    want = golden()[1][name]
    assert {k: list(v.shape) for k, v in sorted(model.state_dict().items())} == want
    wrapped = cfg["model"]["augment_wrapper"]
    # (by name: a test that imports a submodule through the ``k_diffusion_amd`` alias leaves a second copy of its classes behind)
    assert any(c.__name__ == "KarrasAugmentWrapper" for c in type(model).__mro__) == wrapped
    inner = model.inner_model if wrapped else model
    assert type(inner).__name__ == "ImageDenoiserModelV1"
    pre = "inner_model." if wrapped else ""
    assert want[pre + "mapping_cond.weight"] == [64, 9] if wrapped else pre + "mapping_cond.weight" not in want
    assert want[pre + "u_net.d_blocks.1.0.kernel"] == [4, 4] and want[pre + "timestep_embed.weight"] == [32, 1]
    # a reference-layout state dict (plain tensors under the reference's names) loads, strictly
    fresh = KD.config.make_model(cfg)
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in fresh.state_dict().items())
    # every tensor the reference zero-initialises is non-zero under synth
    for k, v in sd.items():
        assert v.abs().max() > 0, k
    # param_groups: weights of mapping / u_net decay, the rest does not (image_v1.py:117-133)
    groups = model.param_groups(3e-4)
    names = {id(p): n for n, p in inner.named_parameters()}
    assert len(groups) == 2 and groups[0]["lr"] == 3e-4 and groups[1]["weight_decay"] == 0.0 and "weight_decay" not in groups[0]
    wd = {names[id(p)] for p in groups[0]["params"]}
    assert wd == {n for n in names.values() if (n.startswith("mapping") or n.startswith("u_net")) and n.endswith(".weight")}
    assert len(groups[0]["params"]) + len(groups[1]["params"]) == len(names)
    # ("mapping_cond.weight" starts with "mapping" too: it decays in the reference, and here)
    assert "proj_in.weight" not in wd and "mapping.0.bias" not in wd and "mapping.0.weight" in wd and ("mapping_cond.weight" in wd) == wrapped


def test_reference_constructor_signature(KD):
    import inspect
    got = [(p.name, p.default) for p in inspect.signature(KD.models.ImageDenoiserModelV1.__init__).parameters.values()][1:]
    assert got == [("c_in", inspect.Parameter.empty), ("feats_in", inspect.Parameter.empty), ("depths", inspect.Parameter.empty),
                   ("channels", inspect.Parameter.empty), ("self_attn_depths", inspect.Parameter.empty), ("cross_attn_depths", None),
                   ("mapping_cond_dim", 0), ("unet_cond_dim", 0), ("cross_cond_dim", 0), ("dropout_rate", 0.), ("patch_size", 1), ("skip_stages", 0),
                   ("has_variance", False)]


@pytest.mark.parametrize("field,value", [("patch_size", 2), ("skip_stages", 1), ("has_variance", True), ("cross_cond_dim", 768), ("unet_cond_dim", 3),
                                         ("channels", [64, 96]), ("channels", [32, 64])])
def test_refusals_name_the_field(KD, field, value):
    m = dict(ur.UNET_A["model"], **{field: value})
    cfg = KD.config.load_config({"model": m, "dataset": ur.UNET_A["dataset"]})
    with pytest.raises(ValueError, match=field):
        KD.config.make_model(cfg)


def test_sampling_only(KD):
    _, model, _ = built("unet_b")
    x, sigma, _ = ur.inputs("unet_b")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            model(x, sigma)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            KD.Denoiser(model, 0.5)(x, sigma)
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model(x.clone().requires_grad_(True), sigma)
    trainable = KD.config.make_model(built("unet_b")[0])
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        trainable(x, sigma)
    with pytest.raises(ValueError, match="skip_stages"):
        model.set_skip_stages(1)
    with pytest.raises(ValueError, match="patch_size"):
        model.set_patch_size(2)
    with pytest.raises(ValueError, match="unsupported model type image_transformer_v1"):
        KD.config.make_model(KD.config.load_config({"model": {"type": "image_transformer_v1", "width": 64}, "dataset": {"num_classes": 0}}))
    src = open(os.path.join(REPO, "train.py")).read()
    assert re.search(r"model_config\['type'\] == 'image_v1':\s+raise NotImplementedError", src)


def test_layers_gains_none_of_the_pinned_names(KD):
    assert not PINNED & set(vars(KD.layers))
    import inspect
    ops_public = {n for n, f in vars(KD.ops).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == KD.ops.__name__}
    assert not ops_public & {"conv2d", "pack_conv", "groupnorm_stats", "adagn_apply", "down2", "up2", "unet_in", "unet_out", "cond_mlp"}
    assert all(callable(getattr(KD.unet_ops, n)) for n in ("conv2d", "pack_conv", "groupnorm_stats", "adagn_apply", "down2", "up2", "unet_in",
                                                            "unet_out", "cond_mlp"))


def test_signatures_and_header_agree_for_the_new_entry_points(KD):
    from tests.test_host_cpu import header_prototypes
    from tests.helpers import source_options
    protos = header_prototypes()
    nat = KD._native
    for name, n_args in NEW_ENTRY_POINTS.items():
        assert protos[name] == n_args == len(nat.SIGNATURES[name]), name
        assert nat.SIGNATURES[name][-1] is C.c_void_p and name not in nat.RUN_LIST_OPS
        assert hasattr(nat.lib(), name)
    # pointer / int / float kinds against the header's declaration
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "kdiff_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        kinds = [C.c_void_p if "*" in a else (C.c_float if a.strip().startswith("float") else C.c_int) for a in decl.split(",")]
        assert kinds == nat.SIGNATURES[name], name
    # the new kernels read no library option
    csrc = os.path.join(REPO, "k-diffusion_amd", "csrc")
    for fn in ("conv_x3.hip", "unet_f32.hip"):
        assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)", open(os.path.join(csrc, fn)).read()), fn
    assert source_options()

"""bf16 weight-gradient arithmetic of the image_v1 U-Net and its command line, the parts that need no GPU: the fifth header
(include/kdiff_unet_mixed.h) against its binding table (``_native.MIXED_SIGNATURES``) with the four pinned tables left as they are,
``set_wgrad_arithmetic`` on the bare and the wrapped model, train.py's ``check_model_config`` and the golden of the reference's own bf16 error
(tests/golden/unet_wgrad_bf16.json)."""
import ctypes as C
import importlib.util
import json
import math
import os
import re

import pytest

from tests import unet_ref as ur
from tests.test_unet_cpu import built
from tests.test_unet_drop_cpu import _kind

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_unet_mixed.h")
ENTRY_POINTS = {"kd_conv2d_wgrad_bf16": 17}
WEIGHTINGS = ("karras", "soft-min-snr")


def header_parameters(path=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kd_\w+)\s*\((.*?)\)\s*;", src, flags=re.S):
        out[name] = [tuple(re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a).groups()) for a in args.split(",")]
    return out


def test_the_library_exports_and_binds_what_the_header_declares(KD):
    nat = KD._native
    params = header_parameters()
    assert sorted(params) == sorted(ENTRY_POINTS) == sorted(nat.MIXED_SIGNATURES) == sorted(nat.MIXED_RESTYPES)
    parsed = KD._abi.parse(open(HEADER).read())
    assert not parsed.structs and not parsed.constants
    lib = nat.lib()
    for name, n_args in ENTRY_POINTS.items():
        kinds = [_kind(t) for t, _ in params[name]]
        assert len(kinds) == n_args and kinds == nat.MIXED_SIGNATURES[name] == parsed.signatures[name], name
        assert kinds[-1] is C.c_void_p and params[name][-1][1] == "stream"
        fn = getattr(lib, name)                                        # exported ...
        assert list(fn.argtypes) == kinds and fn.restype is C.c_int    # ... and bound with the parsed types
    # the argument list is kd_conv2d_wgrad_x3's, name for name and type for type
    x3 = header_parameters(os.path.join(REPO, "include", "kdiff_unet_train.h"))["kd_conv2d_wgrad_x3"]
    assert [(t.strip(), n) for t, n in params["kd_conv2d_wgrad_bf16"]] == [(t.strip(), n) for t, n in x3]
    # the other four tables stay what they were: none of the new names, and no run-list op for them
    others = set(nat.SIGNATURES) | set(nat.GRAD_SIGNATURES) | set(nat.TRAIN_SIGNATURES) | set(nat.DROP_SIGNATURES) | set(nat.RUN_LIST_OPS)
    assert not set(ENTRY_POINTS) & others
    for header in ("kdiff_hip.h", "kdiff_unet_grad.h", "kdiff_unet_train.h", "kdiff_unet_drop.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in ENTRY_POINTS)
    # the new kernel's file reads no library option and calls no atomic, and neither does the shared second pass
    csrc = os.path.join(REPO, "k-diffusion_amd", "csrc")
    for src in ("conv_wgrad_bf16.hip", "conv_wgrad_reduce.h"):
        assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)|\batomic\w*\s*\(", open(os.path.join(csrc, src)).read()), src
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^OBJS := .*\bconv_wgrad_bf16\.o\b", make, flags=re.M)
    assert re.search(r"conv_wgrad_bf16\.o:.*kdiff_unet_mixed\.h", make)
    run_list = open(os.path.join(csrc, "run_list.cpp")).read()
    assert "conv2d_wgrad_bf16" not in run_list
    # the wrapper is unet_ops.conv2d_wgrad's ``bf16`` argument, off by default
    import inspect
    assert inspect.signature(KD.unet_ops.conv2d_wgrad).parameters["bf16"].default is False


def test_set_wgrad_arithmetic_on_the_bare_and_the_wrapped_model(KD):
    bare = KD.config.make_model(built("unet_b")[0])
    before = sorted(bare.state_dict())
    assert bare.wgrad_arithmetic is None
    assert bare.set_wgrad_arithmetic("bf16") is bare and bare.wgrad_arithmetic == "bf16"
    assert sorted(bare.state_dict()) == before, "the setting is not part of the state_dict"
    assert bare.set_wgrad_arithmetic(None) is bare and bare.wgrad_arithmetic is None
    assert bare.set_wgrad_arithmetic("bf16").set_wgrad_arithmetic().wgrad_arithmetic is None
    for bad in ("fp16", "BF16", True, 16, "split3"):
        with pytest.raises(ValueError, match=r"ImageDenoiserModelV1\.set_wgrad_arithmetic"):
            bare.set_wgrad_arithmetic(bad)
        assert bare.wgrad_arithmetic is None
    wrapped = KD.config.make_model(built("unet_a")[0])
    assert hasattr(wrapped, "inner_model")
    keys = sorted(wrapped.state_dict())
    assert wrapped.set_wgrad_arithmetic("bf16") is wrapped and wrapped.inner_model.wgrad_arithmetic == "bf16"
    assert sorted(wrapped.state_dict()) == keys
    assert wrapped.set_wgrad_arithmetic(None) is wrapped and wrapped.inner_model.wgrad_arithmetic is None
    with pytest.raises(ValueError, match=r"ImageDenoiserModelV1\.set_wgrad_arithmetic"):
        wrapped.set_wgrad_arithmetic("fp8")
    # train.py's dropout opt-in test serves both families: the U-Net, bare and wrapped, names its one rate
    assert bare._dropout_rates() == [("dropout_rate", 0.0)] and wrapped._dropout_rates() == wrapped.inner_model._dropout_rates()
    raw = json.loads(json.dumps(ur.CONFIGS["unet_a"]))
    raw["model"]["dropout_rate"] = 0.05
    dropping = KD.config.make_model(KD.config.load_config(raw))
    assert any(rate > 0 for _, rate in dropping._dropout_rates()) and not any(rate > 0 for _, rate in wrapped._dropout_rates())


@pytest.fixture(scope="module")
def train(KD):
    spec = importlib.util.spec_from_file_location("kd_train_script_mixed", os.path.join(REPO, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the model sections of the four image_v1 configs the reference ships (config_mnist, config_cifar10, config_32x32_small,
# config_32x32_small_butterflies: the last three share one model), restated here value for value
_SHIPPED_COMMON = {"type": "image_v1", "patch_size": 1, "mapping_out": 256, "depths": [2, 4, 4], "has_variance": False, "loss_config": "karras",
                   "loss_weighting": "soft-min-snr", "dropout_rate": 0.05, "augment_wrapper": True, "augment_prob": 0.12, "sigma_min": 1e-2,
                   "sigma_max": 80, "sigma_sample_density": {"type": "cosine-interpolated"}}
SHIPPED = {
    "config_mnist": (dict(_SHIPPED_COMMON, input_channels=1, input_size=[28, 28], channels=[128, 128, 256], self_attn_depths=[False, False, True],
                          sigma_data=0.6162), {"type": "mnist", "location": "data"}),
    "config_cifar10": (dict(_SHIPPED_COMMON, input_channels=3, input_size=[32, 32], channels=[128, 256, 512], self_attn_depths=[False, True, True],
                            sigma_data=0.5), {"type": "cifar10", "location": "data"}),
    "config_32x32_small": (dict(_SHIPPED_COMMON, input_channels=3, input_size=[32, 32], channels=[128, 256, 512],
                                self_attn_depths=[False, True, True], sigma_data=0.5), {"type": "imagefolder", "location": "/path/to/dataset"}),
    "config_32x32_small_butterflies": (dict(_SHIPPED_COMMON, input_channels=3, input_size=[32, 32], channels=[128, 256, 512],
                                            self_attn_depths=[False, True, True], sigma_data=0.5),
                                       {"type": "imagefolder", "location": "/path/to/dataset"}),      # shipped as a huggingface dataset: exported
}


def _config(KD, model, dataset):
    return KD.config.load_config({"model": json.loads(json.dumps(model)), "dataset": dict(dataset)})


@pytest.mark.parametrize("name", sorted(SHIPPED))
def test_check_model_config_accepts_the_shipped_configs(KD, train, name):
    config = _config(KD, *SHIPPED[name])
    assert train.check_model_config(config) is None
    train.check_dataset_config(config, 0)                              # and the data path takes them: a bare or wrapped U-Net has 0 class rows


def test_check_model_config_refuses_by_name(KD, train):
    model, dataset = SHIPPED["config_cifar10"]
    with pytest.raises(NotImplementedError, match=r"dataset\.num_classes > 0.*image_v1.*class_cond"):
        train.check_model_config(_config(KD, model, dict(dataset, num_classes=10)))
    with pytest.raises(NotImplementedError, match=r"augment_prob > 0.*augment_wrapper.*aug_cond"):
        train.check_model_config(_config(KD, dict(model, augment_wrapper=False), dataset))
    assert train.check_model_config(_config(KD, dict(model, augment_wrapper=False, augment_prob=0.0), dataset)) is None
    with pytest.raises(ValueError, match=r"input size 28x28: level 2 is 7x7.*cannot halve"):
        train.check_model_config(_config(KD, dict(model, input_size=[28, 28], depths=[1, 1, 1, 1], channels=[64, 64, 64, 64],
                                                  self_attn_depths=[False] * 4), dataset))
    with pytest.raises(ValueError, match=r"input size 30x30: level 1 is 15x15"):
        train.check_model_config(_config(KD, dict(model, input_size=[30, 30]), dataset))
    # the constructor's refusals stay the constructor's, by field name
    for field, value in (("patch_size", 2), ("skip_stages", 1), ("has_variance", True), ("cross_cond_dim", 8), ("unet_cond_dim", 3)):
        config = _config(KD, dict(model, **{field: value}), dataset)
        assert train.check_model_config(config) is None
        with pytest.raises(ValueError, match=field):
            KD.config.make_model(config)
    with pytest.raises(ValueError, match="multiple of 64"):
        KD.config.make_model(_config(KD, dict(model, channels=[96, 256, 512]), dataset))
    # the transformer's configs pass through untouched, class-conditional ones included
    from tests.golden import cases
    raw = cases.raw_config("tiny_global")
    raw.setdefault("dataset", {})["num_classes"] = 10
    assert train.check_model_config(KD.config.load_config(raw)) is None
    # ... and the command line no longer refuses the family before the device check
    src = open(os.path.join(REPO, "train.py")).read()
    assert "does not train the U-Net yet" not in src
    assert src.index("check_model_config(config)\n") < src.index("torch.cuda.is_available()")


def test_the_golden_names_every_parameter(KD):
    gold = json.load(open(os.path.join(REPO, "tests", "golden", "unet_wgrad_bf16.json")))
    assert sorted(gold) == sorted(ur.CONFIGS)
    for name in ur.CONFIGS:
        model = KD.config.make_model(built(name)[0])
        names = sorted(k for k, _ in model.named_parameters())
        assert len(names) == {"unet_a": 84, "unet_b": 72}[name]
        assert sorted(gold[name]) == sorted(WEIGHTINGS)
        for weighting in WEIGHTINGS:
            err = gold[name][weighting]
            assert sorted(err) == names, (name, weighting)
            assert all(isinstance(v, float) and math.isfinite(v) and 0 < v < 1 for v in err.values())

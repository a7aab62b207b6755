"""bf16 convolution arithmetic of the image_v1 U-Net's sampling forward, the parts that need no GPU: the sixth header (include/kdiff_unet_bf16.h)
against its binding table (``_native.UNET_BF16_SIGNATURES``) with the five older tables left as they are, ``unet_ops.conv2d``'s ``bf16``
argument, ``set_conv_arithmetic`` on the bare and the wrapped model, ``sample.py --unet-arithmetic`` on a transformer config and the golden of
the reference's own autocast error (tests/golden/unet_bf16.safetensors)."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

from tests import unet_ref as ur
from tests.test_unet_cpu import built
from tests.test_unet_drop_cpu import _kind
from tests.test_unet_mixed_cpu import header_parameters

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_unet_bf16.h")
ENTRY_POINTS = {"kd_conv2d_bf16": 15}
OLDER_HEADERS = ("kdiff_hip.h", "kdiff_unet_grad.h", "kdiff_unet_train.h", "kdiff_unet_drop.h", "kdiff_unet_mixed.h")


def test_the_library_exports_and_binds_what_the_header_declares(KD):
    nat = KD._native
    params = header_parameters(HEADER)
    assert nat.UNET_BF16_HEADER_PATH == HEADER
    assert sorted(params) == sorted(ENTRY_POINTS) == sorted(nat.UNET_BF16_SIGNATURES) == sorted(nat.UNET_BF16_RESTYPES)
    parsed = KD._abi.parse(open(HEADER).read())
    assert not parsed.structs and not parsed.constants
    lib = nat.lib()
    for name, n_args in ENTRY_POINTS.items():
        kinds = [_kind(t) for t, _ in params[name]]
        assert len(kinds) == n_args and kinds == nat.UNET_BF16_SIGNATURES[name] == parsed.signatures[name], name
        assert kinds[-1] is C.c_void_p and params[name][-1][1] == "stream"
        fn = getattr(lib, name)                                        # exported ...
        assert list(fn.argtypes) == kinds and fn.restype is C.c_int    # ... and bound with the parsed types
    # the argument list is kd_conv2d_x3's, name for name and type for type
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "kdiff_hip.h")).read(), flags=re.S)
    (args,) = re.findall(r"\bint\s+kd_conv2d_x3\s*\((.*?)\)\s*;", main, flags=re.S)
    x3 = [tuple(re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a).groups()) for a in args.split(",")]
    assert [(t.strip(), n) for t, n in params["kd_conv2d_bf16"]] == [(t.strip(), n) for t, n in x3]
    assert [n for _, n in x3] == ["x", "ldx", "wp", "bias", "res", "ldr", "y", "ldy", "batch", "H", "W", "c_in", "c_out", "ks", "stream"]


def test_the_older_tables_and_the_run_list_do_not_name_it(KD):
    nat = KD._native
    others = (set(nat.SIGNATURES) | set(nat.GRAD_SIGNATURES) | set(nat.TRAIN_SIGNATURES) | set(nat.DROP_SIGNATURES) | set(nat.MIXED_SIGNATURES)
              | set(nat.RUN_LIST_OPS))
    assert not set(ENTRY_POINTS) & others
    assert sorted(nat.MIXED_SIGNATURES) == ["kd_conv2d_wgrad_bf16"]
    for header in OLDER_HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
        assert not any(re.search(r"\b" + n + r"\s*\(", text) for n in ENTRY_POINTS), header
    run_list = open(os.path.join(REPO, "k-diffusion_amd", "csrc", "run_list.cpp")).read()
    assert "conv2d_bf16" not in run_list
    assert not any("conv2d_bf16" in line for line in open(os.path.join(REPO, "include", "kdiff_options.def")))


def test_the_kernel_file_reads_no_option_and_calls_no_atomic():
    csrc = os.path.join(REPO, "k-diffusion_amd", "csrc")
    src = open(os.path.join(csrc, "conv_bf16.hip")).read()
    assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)|\batomic\w*\s*\(", src)
    assert '#include "../../include/kdiff_unet_bf16.h"' in src and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" in src
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^OBJS := .*\bconv_bf16\.o\b", make, flags=re.M)
    assert re.search(r"conv_bf16\.o:.*kdiff_unet_bf16\.h", make)


def test_the_wrapper_argument(KD):
    sig = inspect.signature(KD.unet_ops.conv2d).parameters
    assert sig["bf16"].default is False
    # the dual pass and the training loss stay fp32-grade: refused by name, before any tensor is looked at
    for other in ("bias_batch", "chan_scale"):
        with pytest.raises(ValueError, match=other):
            KD.unet_ops.conv2d(None, torch.zeros(64, 64, 1, 1), 1, 1, 1, bf16=True, **{other: 1})
    # nothing new in ops.py: the public list there is pinned by tests/test_guard_cpu.py
    assert not hasattr(KD.ops, "conv2d_bf16")


def test_set_conv_arithmetic_on_the_bare_and_the_wrapped_model(KD):
    bare = KD.config.make_model(built("unet_b")[0])
    before = sorted(bare.state_dict())
    assert bare.conv_arithmetic is None
    assert bare.set_conv_arithmetic("bf16") is bare and bare.conv_arithmetic == "bf16"
    assert sorted(bare.state_dict()) == before, "the setting is not part of the state_dict"
    assert bare.set_conv_arithmetic(None) is bare and bare.conv_arithmetic is None
    assert bare.set_conv_arithmetic("bf16").set_conv_arithmetic().conv_arithmetic is None
    for bad in ("fp16", "BF16", True, 16, "split3", "fp8"):
        with pytest.raises(ValueError, match=r"ImageDenoiserModelV1\.set_conv_arithmetic"):
            bare.set_conv_arithmetic(bad)
        assert bare.conv_arithmetic is None
    assert bare.wgrad_arithmetic is None, "the two settings are separate"
    wrapped = KD.config.make_model(built("unet_a")[0])
    assert hasattr(wrapped, "inner_model")
    keys = sorted(wrapped.state_dict())
    assert wrapped.set_conv_arithmetic("bf16") is wrapped and wrapped.inner_model.conv_arithmetic == "bf16"
    assert sorted(wrapped.state_dict()) == keys
    assert wrapped.set_conv_arithmetic(None) is wrapped and wrapped.inner_model.conv_arithmetic is None
    with pytest.raises(ValueError, match=r"ImageDenoiserModelV1\.set_conv_arithmetic"):
        wrapped.set_conv_arithmetic("fp8")


def test_a_change_of_the_setting_drops_the_plans(KD):
    model = KD.config.make_model(built("unet_b")[0])
    plans = model._plans
    key = (2, 28, 28, "cpu")

    def plant():
        plans[key] = object()                                         # stands for a cached launch plan (one has no release())
    plant()
    model.set_conv_arithmetic(None)                                   # no change: kept
    assert list(plans) == [key]
    model.set_conv_arithmetic("bf16")
    assert not plans and model._plans is plans, "the sampling plans go, the dict stays the model's"
    plant()
    model.set_conv_arithmetic("bf16")                                 # no change again
    assert list(plans) == [key]
    model.set_conv_arithmetic(None)
    assert not plans
    # the plan-cache key stays (batch, H, W, device): the setting is not in it
    src = inspect.getsource(type(model)._plan)
    assert "key = (B, H, W, str(device))" in src


def test_sample_py_refuses_the_flag_for_a_transformer_config(KD, tmp_path, capsys):
    import sample
    from tests.golden import cases
    (tmp_path / "hdit.json").write_text(json.dumps(cases.raw_config("tiny_global")))
    with pytest.raises(SystemExit) as e:
        sample.parse(["--config", str(tmp_path / "hdit.json"), "--random-weights", "--unet-arithmetic", "bf16"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--unet-arithmetic" in err and "KDIFF_GEMM" in err and "image_transformer_v2" in err, err
    with pytest.raises(SystemExit) as e:                              # and only bf16 is a choice
        sample.parse(["--config", str(tmp_path / "hdit.json"), "--random-weights", "--unet-arithmetic", "fp16"])
    assert e.value.code == 2
    capsys.readouterr()
    # an image_v1 config passes the parser, with and without the flag
    (tmp_path / "unet.json").write_text(json.dumps(ur.UNET_B))
    assert sample.parse(["--config", str(tmp_path / "unet.json"), "--random-weights", "--unet-arithmetic", "bf16"]).unet_arithmetic == "bf16"
    assert sample.parse(["--config", str(tmp_path / "unet.json"), "--random-weights"]).unet_arithmetic is None
    assert sample.parse(["--config", str(tmp_path / "hdit.json"), "--random-weights"]).unet_arithmetic is None


def test_the_golden_holds_the_references_autocast_outputs():
    from safetensors.torch import load_file
    gold = load_file(os.path.join(REPO, "tests", "golden", "unet_bf16.safetensors"))
    fp32 = load_file(os.path.join(REPO, "tests", "golden", "unet_v1.safetensors"))
    assert sorted(gold) == sorted(name + ".out_autocast_bf16" for name in ur.CONFIGS)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "unet_bf16.safetensors")) < 64 * 1024
    for name in ur.CONFIGS:
        out, ref = gold[name + ".out_autocast_bf16"], fp32[name + ".out"]
        assert out.dtype == torch.float32 and out.shape == ref.shape and bool(torch.isfinite(out).all())
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        print(f"{name}: the reference under autocast(bf16) is {err:.3e} (max norm, relative) from its fp32 output")
        assert 1e-4 < err < 5e-2, "a bf16 forward's distance from the fp32 one"

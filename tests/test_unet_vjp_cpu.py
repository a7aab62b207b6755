"""The reverse (VJP) pass of the image_v1 U-Net without a GPU: the ABI of its four entry points, which live in a header of their own
(include/kdiff_unet_grad.h) and a binding table of their own (``_native.GRAD_SIGNATURES``) so that the main header's table stays as it is, the
wrappers' signatures against the header's parameter lists, and the refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from tests import unet_ref as ur
from tests.test_unet_cpu import built

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kdiff_unet_grad.h")
# entry point -> (argument count, its wrapper in unet_ops, the pointer parameter the wrapper calls ``out``)
ENTRY_POINTS = {"kd_adagn_vjp_stats_f32": (14, "adagn_vjp_stats", "gstats"), "kd_adagn_vjp_apply_f32": (18, "adagn_vjp_apply", "g_x"),
                "kd_down2_vjp_f32": (10, "down2_vjp", "g_x"), "kd_up2_vjp_f32": (10, "up2_vjp", "g_x")}


def header_parameters():
    """name -> [(type text, parameter name)] of every prototype the header declares."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kd_\w+)\s*\((.*?)\)\s*;", src, flags=re.S):
        out[name] = [tuple(re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", a).groups()) for a in args.split(",")]
    return out


def test_the_library_exports_and_binds_what_the_header_declares(KD):
    nat = KD._native
    params = header_parameters()
    assert sorted(params) == sorted(ENTRY_POINTS) == sorted(nat.GRAD_SIGNATURES) == sorted(nat.GRAD_RESTYPES)
    parsed = KD._abi.parse(open(HEADER).read())
    assert not parsed.structs and not parsed.constants
    lib = nat.lib()
    for name, (n_args, _, _) in ENTRY_POINTS.items():
        kinds = [C.c_void_p if "*" in t else (C.c_float if t.strip().startswith("float") else C.c_int) for t, _ in params[name]]
        assert len(kinds) == n_args and kinds == nat.GRAD_SIGNATURES[name] == parsed.signatures[name], name
        assert kinds[-1] is C.c_void_p and params[name][-1][1] == "stream"
        fn = getattr(lib, name)                                        # exported ...
        assert list(fn.argtypes) == kinds and fn.restype is C.c_int    # ... and bound with the parsed types
    # the main header's tables stay what they were: none of the new names, and no run-list op for them
    assert not set(ENTRY_POINTS) & set(nat.SIGNATURES) and not set(ENTRY_POINTS) & set(nat.RUN_LIST_OPS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "kdiff_hip.h")).read(), flags=re.S)
    assert not any(re.search(r"\b" + n + r"\s*\(", main) for n in ENTRY_POINTS)


def test_wrappers_agree_with_the_header(KD):
    """A wrapper takes the header's pointer operands in the header's order under the header's names (its result as ``out``), and the header's
    flags by name; nothing of the kind lands in ``ops`` (tests/test_guard_cpu.py wants a case in tests/test_bounds_gpu.py for everything there)."""
    uo = KD.unet_ops
    params = header_parameters()
    for name, (_, wrapper, result) in ENTRY_POINTS.items():
        sig = list(inspect.signature(getattr(uo, wrapper)).parameters)
        pointers = [p for t, p in params[name] if "*" in t and p != "stream"]
        assert result in pointers, name
        operands = [p for p in pointers if p != result]
        assert sig[:len(operands)] == operands, (name, sig, operands)
        assert "out" in sig
        for flag in ("gelu", "accumulate"):
            assert (flag in sig) == (flag in [p for _, p in params[name]]), (name, flag)
    for wrapper in [w for _, w, _ in ENTRY_POINTS.values()] + ["pack_conv_dgrad", "conv2d_dgrad"]:
        assert callable(getattr(uo, wrapper)) and wrapper not in vars(KD.ops)
    # the new kernels read no library option and call no atomic
    src = open(os.path.join(REPO, "k-diffusion_amd", "csrc", "unet_vjp_f32.hip")).read()
    assert not re.findall(r"\bopt(?:_or)?\(|\bcode_warm\(\)|\batomic\w*\s*\(", src)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_vjp_refusals_without_a_device(KD, name):
    _, model, _ = built(name)
    x, sigma, aug = ur.inputs(name)
    kw = {} if aug is None else {"aug_cond": aug}
    for call in (model.forward_vjp, KD.Denoiser(model, 0.5).forward_vjp):
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(x, sigma, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                # grad mode alone changes nothing
            call(x, sigma, **kw)
        with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
            call(x.clone().requires_grad_(True), sigma, **kw)
        with torch.no_grad():
            with pytest.raises(ValueError, match="unet_cond"):
                call(x, sigma, unet_cond=x, **kw)
    trainable = KD.config.make_model(built(name)[0])
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        trainable.forward_vjp(x, sigma, **kw)
    # the autograd route stays refused: forward_vjp is an explicit method, not a backward pass behind forward
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model(x.clone().requires_grad_(True), sigma, **kw)


def test_denoiser_needs_a_rule_from_the_inner_model(KD):
    class Plain(torch.nn.Module):
        def forward(self, x, sigma):
            return x
    with pytest.raises(NotImplementedError, match="Plain has no forward_vjp rule"):
        KD.Denoiser(Plain(), 0.5).forward_vjp(torch.zeros(1, 3, 8, 8), torch.ones(1))
    with pytest.raises(NotImplementedError, match="Plain has no forward_jvp rule"):      # the wording it follows
        KD.Denoiser(Plain(), 0.5).forward_jvp(torch.zeros(1, 3, 8, 8), torch.ones(1), torch.zeros(1, 3, 8, 8))

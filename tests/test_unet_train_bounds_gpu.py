"""Guard bands (tests/guard.py, as tests/test_bounds_gpu.py) around the operands of the image_v1 U-Net's parameter-gradient entry points
(include/kdiff_unet_train.h) at ragged and strided shapes: nothing is read or written outside a tensor -- the workspaces included, which are
handed in guarded and must be written in full -- and the result is the ordinary call's, bit for bit, under both guard fills.  The entry points
are called through the C ABI directly, so that the workspace is the test's."""
import ctypes as C

import pytest
import torch
from torch.nn import functional as F

from tests.guard import Case, run_case
from tests.test_unet_gpu import DEV, F32, _lib_call, _p, adagn_expr, rn, tokens
from tests.test_unet_train_gpu import SUM_BOUND, WGRAD_BOUND, wgrad_reference

pytestmark = pytest.mark.gpu


def _wgrad_case(B, hw, ci, co, ks, strided):
    def make(env):
        H, W = hw
        a, gy, ref = wgrad_reference(B, hw, ci, co, ks)
        per, n = env.unet_ops.conv_wgrad_chunks(B, H, W, ci, co)
        at, gt = tokens(a), tokens(gy)
        if strided:                                                     # the operands are the right halves of buffers of twice the width
            at, gt = torch.cat([rn(*at.shape, seed=1), at], dim=1), torch.cat([rn(*gt.shape, seed=2), gt], dim=1)

        def call(T):
            ga, gg = (T["a"][:, ci:], T["g"][:, co:]) if strided else (T["a"], T["g"])
            _lib_call("kd_conv2d_wgrad_x3", _p(gg), T["g"].shape[1], _p(ga), T["a"].shape[1], _p(T["ws"]), _p(T["dw"]), B, H, W, ci, co, ks, 0, per, n, 0)
            return T["dw"], T["ws"]
        return dict(ins={"a": at, "g": gt}, outs={"ws": ((n, ks * ks, co, ci), F32), "dw": ((co, ci, ks, ks), F32)}, call=call,
                    ref=lambda R: (ref, None), tol=[("abs", WGRAD_BOUND * ref.abs().max().item()), None])
    return Case(f"conv2d_wgrad_x3[k{ks},{ci}->{co},B{B},{hw[0]}x{hw[1]}{',strided' if strided else ''}]", "conv2d_wgrad", "conv_wgrad_x3.hip", make,
                kernel="conv2d_wgrad_x3")


def _adagn_wb_case(gelu):
    def make(env):
        B, H, W, chan, groups = 2, 6, 10, 128, 4
        x, w, b, gy = 1.5 * rn(B, chan, H, W, seed=3) + 0.3, 0.5 * rn(B, chan, seed=4), 0.5 * rn(B, chan, seed=5), rn(B, chan, H, W, seed=6)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        ref = torch.cat(torch.autograd.grad(adagn_expr(x.double(), w64, b64, groups, gelu), (w64, b64), gy.double()), dim=1)

        def call(T):
            _lib_call("kd_groupnorm_stats_f32", _p(T["x"]), chan, _p(T["st"]), B, H * W, chan, groups, C.c_float(1e-5))
            _lib_call("kd_adagn_wb_grad_f32", _p(T["x"]), chan, _p(T["st"]), _p(T["wb"]), 2 * chan, _p(T["gy"]), chan, _p(T["gwb"]), 2 * chan, B, H * W,
                      chan, groups, int(gelu))
            return T["gwb"]
        return dict(ins={"x": tokens(x), "wb": torch.cat([w, b], 1), "gy": tokens(gy)}, outs={"st": ((B, groups, 4), F32), "gwb": ((B, 2 * chan), F32)},
                    call=call, ref=lambda R: ref, tol=("abs", SUM_BOUND * ref.abs().max().item()))
    return Case(f"adagn_wb_grad[2,6x10,128,{'gelu' if gelu else 'plain'}]", "adagn_wb_grad", "unet_train_f32.hip", make, kernel="adagn_wb_grad_f32")


def _gelu_vjp_case():
    def make(env):
        pre, gy = 3.0 * rn(3, 70, seed=1), rn(3, 70, seed=2)
        p64 = pre.double().requires_grad_(True)
        ref = torch.autograd.grad(F.gelu(p64), p64, gy.double())[0]

        def call(T):
            _lib_call("kd_gelu_vjp_f32", _p(T["pre"]), _p(T["gy"]), _p(T["gx"]), 210)
            return T["gx"]
        return dict(ins={"pre": pre, "gy": gy}, outs={"gx": ((3, 70), F32)}, call=call, ref=lambda R: ref, tol=("abs", SUM_BOUND * ref.abs().max().item()))
    return Case("gelu_vjp[3x70]", "gelu_vjp", "unet_train_f32.hip", make, kernel="gelu_vjp_f32")


def _bias_case(layout):
    def make(env):
        B, H, W, chan = 3, 13, 17, 3 if layout == "nchw" else 192      # 663 rows: three runs, the last ragged
        gy = rn(B, chan, H, W, seed=9) + 0.25
        ref = gy.double().sum(dim=(0, 2, 3))
        rows, runs = B * H * W, -(-B * H * W // 256)
        gt = gy if layout == "nchw" else torch.cat([rn(rows, chan, seed=3), tokens(gy)], dim=1)

        def call(T):
            if layout == "nchw":
                _lib_call("kd_bias_grad_f32", _p(T["g"]), 0, _p(T["ws"]), _p(T["out"]), rows, chan, H * W, 0, 0)
            else:
                _lib_call("kd_bias_grad_f32", _p(T["g"][:, chan:]), 2 * chan, _p(T["ws"]), _p(T["out"]), rows, chan, 0, 0, 0)
            return T["out"], T["ws"]
        return dict(ins={"g": gt}, outs={"ws": ((runs, chan), torch.float64), "out": ((chan,), F32)}, call=call, ref=lambda R: (ref, None),
                    tol=[("abs", SUM_BOUND * ref.abs().max().item()), None])
    return Case(f"bias_grad[{layout},663 rows]", "bias_grad", "unet_train_f32.hip", make, kernel="bias_grad_f32")


CASES = [_wgrad_case(2, (12, 20), 64, 128, 3, False), _wgrad_case(2, (12, 20), 64, 128, 3, True), _wgrad_case(3, (7, 7), 128, 64, 3, False),
         _wgrad_case(1, (2, 2), 64, 64, 3, False), _wgrad_case(2, (16, 8), 128, 192, 1, True), _adagn_wb_case(True), _adagn_wb_case(False),
         _gelu_vjp_case(), _bias_case("strided"), _bias_case("nchw")]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")

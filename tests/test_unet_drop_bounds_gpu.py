"""Guard bands (tests/guard.py, as tests/test_unet_train_bounds_gpu.py) around the operands of the image_v1 U-Net's five dropout entry points
(include/kdiff_unet_drop.h) at the ragged and strided shapes of tests/test_unet_drop_gpu.py: nothing is read or written outside a tensor -- the
key, the site triples and the workspaces included -- every output is written in full, and the result is the ordinary call's, bit for bit, under
both guard fills.  The entry points are called through the C ABI directly."""
import pytest
import torch

from tests import unet_drop_ref as dr
from tests.guard import Case, run_case
from tests.test_unet_drop_gpu import (ATTN_B, ATTN_FWD_BOUND, ATTN_NH, ATTN_P, ATTN_SITE, ATTN_VJP_BOUND, CONV_SHAPE, KEYS, attn_drop_expr, attn_mask,
                                      conv_drop_reference, factors, pack_qkv)
from tests.test_unet_gpu import DEV, F32, SPLIT3, _lib_call, _p, rn, tokens

pytestmark = pytest.mark.gpu
I64 = torch.int64


def _args(p):
    import ctypes as C
    import math
    return math.floor(p * 2.0 ** 32), C.c_float(1.0 / (1.0 - p))


def _chan_mask_case(p):
    def make(env):
        B, key = 3, KEYS[1]
        sites = [(dr.SITE | 4, 64), (dr.SITE | 5, 128)]
        layout, width = env.unet_ops.chan_layout(sites)
        ref = torch.from_numpy(factors(torch.cat([torch.from_numpy(dr.chan_keep(key, s, p, B, C)) for s, C in sites], dim=1).numpy(), p))

        def call(T):
            _lib_call("kd_chan_mask_f32", _p(T["key"]), _p(T["sites"]), len(layout), *_args(p), _p(T["table"]), width, B)
            return T["table"]
        return dict(ins={"key": torch.tensor([key], dtype=I64), "sites": torch.tensor(layout, dtype=I64)}, outs={"table": ((B, width), F32)}, call=call,
                    ref=lambda R: ref, ref32=True, tol=0)
    return Case(f"chan_mask[B3,64+128,p{p}]", "chan_mask", "unet_drop_f32.hip", make, kernel="chan_mask_f32")


def _conv_drop_case(ks, bias, residual):
    def make(env):
        B, (H, W), ci, co = CONV_SHAPE["B"], CONV_SHAPE["hw"], CONV_SHAPE["ci"], CONV_SHAPE["co"]
        x, w, b, r, keep, m, ref, bound = conv_drop_reference(ks, bias, residual)
        rows = B * H * W
        # strided operands: x and the residual are the right halves of buffers of twice the width, the site a column range of a wider table
        ins = {"x": torch.cat([rn(rows, ci, seed=1), tokens(x)], dim=1), "w": w, "m": torch.cat([rn(B, 64, seed=2), m, rn(B, 64, seed=3)], dim=1)}
        if bias:
            ins["b"] = b
        if residual:
            ins["r"] = torch.cat([rn(rows, co, seed=4), tokens(r)], dim=1)

        def call(T):
            _lib_call("kd_pack_conv_x3", _p(T["w"]), _p(T["wp"]), co, ci, ks)
            _lib_call("kd_conv2d_x3_drop", _p(T["x"][:, ci:]), 2 * ci, _p(T["wp"]), _p(T.get("b")), _p(T["r"][:, co:]) if residual else None, 2 * co,
                      _p(T["m"][:, 64:]), co + 128, _p(T["y"]), co, B, H, W, ci, co, ks)
            return T["y"]

        def tol(got, want):
            got = got.cpu().double()
            kept = tokens(torch.from_numpy(keep)[:, :, None, None].expand(B, co, H, W))
            err = ((got - want).abs() / tokens(bound))[kept].max().item()
            assert err < SPLIT3, f"{err:.3e} of scale * sum|a||w|"
            assert torch.equal(got[~kept], want[~kept]), "a dropped channel is not the residual (or 0) exactly"
            return err
        return dict(ins=ins, outs={"wp": ((4 * ks * ks * ci * co,), torch.uint8), "y": ((rows, co), F32)}, call=call, ref=lambda R: tokens(ref), tol=tol)
    return Case(f"conv2d_x3_drop[k{ks},64->128,B3,12x20,strided{',bias' if bias else ''}{',res' if residual else ''}]", "conv2d", "conv_x3.hip", make,
                kernel="conv2d_x3_drop")


def _chan_scale_case(inplace):
    def make(env):
        B, H, W, C = 3, 12, 20, 128
        rows = B * H * W
        gy = rn(rows, C, seed=4)
        m = torch.from_numpy(factors(dr.chan_keep(KEYS[0], dr.SITE | 3, 0.25, B, C), 0.25))
        wide = torch.cat([rn(rows, C, seed=5), gy], dim=1)
        table = torch.cat([rn(B, 64, seed=6), m, rn(B, 64, seed=7)], dim=1)
        want = (gy.view(B, H * W, C) * m[:, None, :]).view(rows, C)

        def call(T):
            dst = T["g"][:, C:] if inplace else T["out"]
            _lib_call("kd_chan_scale_f32", _p(T["g"][:, C:]), 2 * C, _p(T["m"][:, 64:]), C + 128, _p(dst), 2 * C if inplace else C, B, H * W, C)
            return T["g"] if inplace else T["out"]
        ref = torch.cat([wide[:, :C], want], dim=1) if inplace else want
        return dict(ins={"g": wide, "m": table}, outs={} if inplace else {"out": ((rows, C), F32)}, inplace=["g"] if inplace else [], call=call,
                    ref=lambda R: ref, ref32=True, tol=0)
    return Case(f"chan_scale[B3,12x20,128,strided,{'in place' if inplace else 'out of place'}]", "chan_scale", "unet_drop_f32.hip", make,
                kernel="chan_scale_f32")


def _attn_operands(T):
    B, nh = ATTN_B, ATTN_NH
    q, k, v = (rn(B, T, nh, 64, seed=s) * sc for s, sc in ((1, 0.6), (2, 0.6), (3, 1.0)))
    return pack_qkv(q, k, v), rn(B, T, nh * 64, seed=4)


def _attn_drop_case(T):
    def make(env):
        B, nh, key = ATTN_B, ATTN_NH, KEYS[1]
        qkv, _ = _attn_operands(T)
        ref = attn_drop_expr(qkv.double(), attn_mask(T, key), nh)

        def call(T_):
            _lib_call("kd_attn_global_drop_f32", _p(T_["qkv"]), _p(T_["out"]), B, T, nh, _p(T_["key"]), ATTN_SITE, *_args(ATTN_P))
            return T_["out"]
        return dict(ins={"qkv": qkv, "key": torch.tensor([key], dtype=I64)}, outs={"out": ((B, T, nh * 64), F32)}, call=call, ref=lambda R: ref,
                    tol=("abs", ATTN_FWD_BOUND * ref.abs().max().item()))
    return Case(f"attn_global_drop[B2,nh2,T{T}]", "attn_global_drop", "vjp_f32.hip", make, kernel="attn_global_drop_f32")


def _attn_drop_vjp_case(T):
    def make(env):
        B, nh, key = ATTN_B, ATTN_NH, KEYS[0]
        qkv, go = _attn_operands(T)
        x64 = qkv.double().requires_grad_()
        ref, = torch.autograd.grad(attn_drop_expr(x64, attn_mask(T, key), nh), x64, go.double())

        def call(T_):
            _lib_call("kd_attn_global_drop_vjp_f32", _p(T_["qkv"]), _p(T_["go"]), _p(T_["gqkv"]), _p(T_["lse"]), _p(T_["dsum"]), B, T, nh, _p(T_["key"]),
                      ATTN_SITE, *_args(ATTN_P))
            return T_["gqkv"], T_["lse"], T_["dsum"]
        return dict(ins={"qkv": qkv, "go": go, "key": torch.tensor([key], dtype=I64)},
                    outs={"gqkv": ((B, T, 3 * nh * 64), F32), "lse": ((B, nh, T), F32), "dsum": ((B, nh, T), F32)}, call=call,
                    ref=lambda R: (ref, None, None), tol=[("abs", ATTN_VJP_BOUND * ref.abs().max().item()), None, None])
    return Case(f"attn_global_drop_vjp[B2,nh2,T{T}]", "attn_global_drop_vjp", "vjp_f32.hip", make, kernel="attn_global_drop_vjp_f32")


CASES = [_chan_mask_case(0.05), _chan_mask_case(0.5), _conv_drop_case(3, True, True), _conv_drop_case(1, True, True), _conv_drop_case(3, False, False),
         _chan_scale_case(False), _chan_scale_case(True), _attn_drop_case(49), _attn_drop_case(80), _attn_drop_vjp_case(49), _attn_drop_vjp_case(80)]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")

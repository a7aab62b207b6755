"""Guard bands (tests/guard.py, as tests/test_unet_mixed_bounds_gpu.py) around x, wp, bias, res and y of ``kd_conv2d_bf16``
(include/kdiff_unet_bf16.h), plain and strided, at the ragged shape, at the 2 x 2 shape and at ks 1: nothing is read or written outside a tensor,
everything inside y is written, and the result is the ordinary call's, bit for bit, under both guard fills.  The entry point is called through
the C ABI directly, on a packed image the test makes itself (``kd_pack_conv_x3`` into a guarded buffer)."""
import pytest
import torch
from torch.nn import functional as F

from tests.guard import Case, run_case
from tests.test_unet_gpu import DEV, F32, _lib_call, _p, rn, tokens

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -21


def _conv_case(B, hw, ci, co, ks, strided):
    def make(env):
        H, W = hw
        seed = 1000 * ks + ci + co + 7 * H + W
        x, w = rn(B, ci, H, W, seed=seed), rn(co, ci, ks, ks, seed=seed + 1) / (ks * ci ** 0.5)
        b, r = rn(co, seed=seed + 2), rn(B, co, H, W, seed=seed + 3)
        xb, wb = x.bfloat16(), w.bfloat16()
        truth = F.conv2d(xb.double(), wb.double(), b.double(), padding=ks // 2) + r.double()
        yard = F.conv2d(xb.float(), wb.float(), b, padding=ks // 2) + r
        scale = F.conv2d(xb.double().abs(), wb.double().abs(), padding=ks // 2)
        bound = max(4 * ((yard.double() - truth).abs() / scale).max().item(), FLOOR)
        xt, rt = tokens(x), tokens(r)
        if strided:                                                     # the operands are the right halves of buffers of twice the width
            xt, rt = torch.cat([rn(*xt.shape, seed=1), xt], dim=1), torch.cat([rn(*rt.shape, seed=2), rt], dim=1)
        ldy = 2 * co if strided else co

        def call(T):
            gx, gr = (T["x"][:, ci:], T["r"][:, co:]) if strided else (T["x"], T["r"])
            gy = T["y"][:, co:] if strided else T["y"]
            if strided:
                T["y"][:, :co] = 0.0                                    # the half beside the output range is the caller's
            _lib_call("kd_pack_conv_x3", _p(T["w"]), _p(T["wp"]), co, ci, ks)
            _lib_call("kd_conv2d_bf16", _p(gx), T["x"].shape[1], _p(T["wp"]), _p(T["b"]), _p(gr), T["r"].shape[1], _p(gy), ldy, B, H, W, ci, co, ks)
            return T["y"], T["wp"]

        def tol(got, want):
            y = got.cpu().double()[:, co:] if strided else got.cpu().double()
            if strided:
                assert bool((got.cpu()[:, :co] == 0).all()), "the columns beside the output range were written"
            err = ((y - want).abs() / tokens(scale)).max().item()
            assert err <= bound, f"{err:.3e} of sum|a^||w^|, bound {bound:.3e}"
            return err
        return dict(ins={"x": xt, "w": w, "b": b, "r": rt}, outs={"wp": ((4 * ks * ks * ci * co,), torch.uint8), "y": ((B * H * W, ldy), F32)},
                    call=call, ref=lambda R: (tokens(truth), None), tol=[tol, None])
    return Case(f"conv2d_bf16[k{ks},{ci}->{co},B{B},{hw[0]}x{hw[1]}{',strided' if strided else ''}]", "conv2d", "conv_bf16.hip", make,
                kernel="conv2d_bf16")


CASES = [_conv_case(2, (12, 20), 64, 128, 3, False), _conv_case(2, (12, 20), 64, 128, 3, True), _conv_case(1, (2, 2), 64, 64, 3, False),
         _conv_case(2, (16, 8), 128, 192, 1, True)]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")

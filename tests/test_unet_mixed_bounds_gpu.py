"""Guard bands (tests/guard.py, as tests/test_unet_train_bounds_gpu.py) around g, a, ws and dw of ``kd_conv2d_wgrad_bf16``
(include/kdiff_unet_mixed.h), plain and strided, at the ragged shape and at the 2 x 2 shape: nothing is read or written outside a tensor -- the
workspace included, which is handed in guarded and must be written in full -- and the result is the ordinary call's, bit for bit, under both
guard fills.  The entry point is called through the C ABI directly, so that the workspace is the test's."""
import pytest
import torch

from tests.guard import Case, run_case
from tests.test_unet_gpu import DEV, F32, _lib_call, _p, rn, tokens
from tests.test_unet_mixed_gpu import rounded_reference

pytestmark = pytest.mark.gpu


def _wgrad_case(B, hw, ci, co, ks, strided):
    def make(env):
        H, W = hw
        a, gy, truth, bound, _ = rounded_reference(B, hw, ci, co, ks)
        per, n = env.unet_ops.conv_wgrad_chunks(B, H, W, ci, co)
        at, gt = tokens(a), tokens(gy)
        if strided:                                                     # the operands are the right halves of buffers of twice the width
            at, gt = torch.cat([rn(*at.shape, seed=1), at], dim=1), torch.cat([rn(*gt.shape, seed=2), gt], dim=1)

        def call(T):
            ga, gg = (T["a"][:, ci:], T["g"][:, co:]) if strided else (T["a"], T["g"])
            _lib_call("kd_conv2d_wgrad_bf16", _p(gg), T["g"].shape[1], _p(ga), T["a"].shape[1], _p(T["ws"]), _p(T["dw"]), B, H, W, ci, co, ks, 0, per, n, 0)
            return T["dw"], T["ws"]
        return dict(ins={"a": at, "g": gt}, outs={"ws": ((n, ks * ks, co, ci), F32), "dw": ((co, ci, ks, ks), F32)}, call=call,
                    ref=lambda R: (truth, None), tol=[("abs", bound), None])
    return Case(f"conv2d_wgrad_bf16[k{ks},{ci}->{co},B{B},{hw[0]}x{hw[1]}{',strided' if strided else ''}]", "conv2d_wgrad", "conv_wgrad_bf16.hip", make,
                kernel="conv2d_wgrad_bf16")


CASES = [_wgrad_case(2, (12, 20), 64, 128, 3, False), _wgrad_case(2, (12, 20), 64, 128, 3, True), _wgrad_case(1, (2, 2), 64, 64, 3, False),
         _wgrad_case(1, (2, 2), 64, 64, 3, True), _wgrad_case(2, (16, 8), 128, 192, 1, True)]


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_guard_bands(KD, c):
    res = run_case(c, "nan", env=KD, device=DEV)
    print(f"{c.name}: errors {['%.2e' % e for e in res.errs]}")

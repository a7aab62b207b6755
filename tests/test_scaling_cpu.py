"""The scaling harness (tests/scaling.py) proves itself, without a GPU: fake ops on the CPU under the relations that tests/test_scaling_gpu.py
declares for the builders whose input names they borrow.  Correct ops satisfy their relations bit for bit; each seeded defect is caught, and by
the relation named for it -- among them a 1e-6 leak from the next row, which the suite's ``relerr`` yardstick at 1e-4 does not see.  Also the
completeness of the declarations: every case of a family carries a relation."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import test_scaling_gpu as sg
from tests.guard import Case
from tests.helpers import relerr
from tests.scaling import LIM, MAG, Relation, describe_mismatch, exponents, factors, run_relation, scale_exact

BF = torch.bfloat16


def rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def split(t):
    hi = t.to(BF).float()
    return hi, (t - hi).to(BF).float()


def matmul(x, w):
    return x @ w.T


def split3(x, w, pair=lambda lo: lo):
    """the restated split3 product; ``pair`` re-pairs A's lo plane with the k axis (the seeded defect)"""
    (xh, xl), (wh, wl) = split(x), split(w)
    return pair(xl) @ wh.T + xh @ wl.T + xh @ wh.T


def lin_case(fn, M=150, N=24, K=40):
    """a fake projection under the names of tests/test_bounds_gpu.py: _lin("plain")"""
    def make(env):
        return dict(ins={"x": rn(M, K, seed=1), "w": rn(N, K, seed=2) / K ** 0.5}, call=lambda T: fn(T["x"], T["w"]))
    return Case(f"linear[plain,exact,M{M},N{N},K{K}]", "linear", "fake", make)


B_, CI, CO, H_, W_ = 3, 8, 6, 5, 6


def conv_fn(leak=0.0):
    def fn(T):
        x = T["x"].view(B_, H_, W_, CI).permute(0, 3, 1, 2)
        y = F.conv2d(x, T["w"], T["b"], padding=1)
        y = y + leak * torch.roll(y, -1, 0)                   # sample b picks up a trace of sample b + 1
        return y.permute(0, 2, 3, 1).reshape(-1, CO) + T["r"]
    return fn


def conv_case(fn):
    """a fake convolution on tokens under the names of tests/test_unet_gpu.py: _conv_case"""
    def make(env):
        return dict(ins={"x": rn(B_ * H_ * W_, CI, seed=3), "w": rn(CO, CI, 3, 3, seed=4) / 8, "b": rn(CO, seed=5), "r": rn(B_ * H_ * W_, CO, seed=6)}, call=fn)
    return Case(f"conv2d_x3[k3,{CI}->{CO},{H_}x{W_}]", "conv2d", "fake", make)


def wgrad_case():
    def fn(T):
        (gh, gl), (ah, al) = split(T["G"]), split(T["A"])
        return gl.T @ ah + gh.T @ al + gh.T @ ah
    return Case("wgrad[plain,split3,M37,N12,K10]", "wgrad", "fake", lambda env: dict(ins={"G": rn(37, 12, seed=1), "A": rn(37, 10, seed=2)}, call=fn))


def attn_case():
    B, T_, nh = 3, 9, 2

    def fn(T):
        q, k, v = (t.transpose(1, 2) for t in T["qkv"].view(B, T_, 3, nh, 64).unbind(2))
        return (torch.softmax(q @ k.transpose(2, 3) / 8, dim=-1) @ v).transpose(1, 2).reshape(B, T_, nh * 64)
    return Case(f"attn_global[exact,1x{T_},nh{nh},B{B},prep=None]", "attn_global", "fake", lambda env: dict(ins={"qkv": rn(B, T_, 3 * nh * 64, seed=1)}, call=fn))


def run(case, name):
    rel, = [r for r in sg.relations_for(case) if r.name == name]
    return run_relation(case, rel)


def names(case):
    return [r.name for r in sg.relations_for(case)]


# ---- correct ops satisfy their relations ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [lin_case(matmul), lin_case(split3), conv_case(conv_fn()), wgrad_case(), attn_case()], ids=["matmul", "split3", "conv2d", "wgrad", "softmax(qk)v"])
def test_correct_ops_satisfy_their_relations(case):
    assert len(names(case)) >= 2
    for name in names(case):
        run(case, name)


def test_relation_sets_of_the_fake_ops():
    assert names(lin_case(matmul)) == ["rows", "cols", "k"]
    assert names(conv_case(conv_fn())) == ["sample", "c_out", "c_in"]
    assert names(wgrad_case()) == ["outer", "pair"]
    assert names(attn_case()) == ["v cols", "v sample"]


# ---- seeded defects ------------------------------------------------------------------------------------------------------------------------------------

def test_leak_from_the_next_row_is_caught_and_invisible_to_relerr():
    leaky = lambda x, w: matmul(x, w) + 1e-6 * torch.roll(matmul(x, w), -1, 0)
    case = lin_case(leaky)
    with pytest.raises(AssertionError, match=r"rows.*elements differ.*dim 0 \(rows / samples\)"):
        run(case, "rows")
    # the point of the file: against fp64 the leaking op passes the suite's yardstick (1e-4 for split3, 2e-5 for exact) by a wide margin
    ins = case.make(None)["ins"]
    err = relerr(leaky(ins["x"], ins["w"]), matmul(ins["x"].double(), ins["w"].double()))
    assert err < 2e-5 < 1e-4, err
    # columns are not mixed: that relation does not see the leak, which is what localises it to the rows
    run(case, "cols")


def test_leak_from_the_next_sample_of_a_convolution_is_caught():
    case = conv_case(conv_fn(leak=1e-6))
    with pytest.raises(AssertionError, match="sample.*elements differ"):
        run(case, "sample")
    run(case, "c_out")
    run(case, "c_in")


def test_absolute_flush_threshold_is_caught():
    flush = lambda x, w: matmul(torch.where(x.abs() < 1e-4, torch.zeros_like(x), x), w)
    with pytest.raises(AssertionError, match="rows.*elements differ"):
        run(lin_case(flush), "rows")
    with pytest.raises(AssertionError, match="k.*elements differ"):
        run(lin_case(flush), "k")


def test_absolute_term_inside_a_sum_is_caught():
    """1e-12 is below half an ulp of every baseline result of order 1, and far above one of a row scaled by 2^-20"""
    plus = lambda x, w: (x[:, :, None] * w.T[None]).sum(1) + 1e-12
    for name in ("rows", "cols"):
        with pytest.raises(AssertionError, match=name + ".*elements differ"):
            run(lin_case(plus), name)


def test_lo_plane_paired_with_the_wrong_k_is_caught_by_the_reduction_axis_relation_only():
    wrong = lambda x, w: split3(x, w, pair=lambda lo: torch.roll(lo, 1, 1))
    case = lin_case(wrong)
    run(case, "rows")
    run(case, "cols")
    with pytest.raises(AssertionError, match="k: result 0 is not the baseline unchanged.*elements differ"):
        run(case, "k")
    ins = case.make(None)["ins"]
    assert relerr(wrong(ins["x"], ins["w"]), matmul(ins["x"].double(), ins["w"].double())) < 1e-2       # (small enough to hide in a bf16 bound)


def test_tile_dependent_summation_order_is_not_flagged():
    """rows from 128 on are summed in the opposite order: another path, equally homogeneous -- a relation compares a row with itself"""
    def tiled(x, w):
        p = x[:, :, None] * w.T[None]
        return torch.cat([p[:128].sum(1), p[128:].flip(1).cumsum(1)[:, -1]])
    case = lin_case(tiled)
    ins = case.make(None)["ins"]
    assert not torch.equal(tiled(ins["x"], ins["w"])[128:], (ins["x"][:, :, None] * ins["w"].T[None]).sum(1)[128:])       # it IS another order
    for name in names(case):
        run(case, name)


# ---- the harness's own conditions ----------------------------------------------------------------------------------------------------------------------

def test_exponents_put_the_extremes_on_neighbours():
    for n in (2, 3, 150):
        k = exponents(n, 1)
        assert int(k[0]) == LIM and int(k[1]) == -LIM and int(k.abs().max()) <= LIM and torch.equal(k, exponents(n, 1))
    assert int(exponents(1, 1)[0]) == LIM and int(exponents(5, 2, 8).abs().max()) == 8
    assert torch.equal(factors(4, 3), torch.ldexp(torch.ones(4, dtype=torch.float64), exponents(4, 3)))


def test_conditions_are_asserted_before_anything_runs():
    called = []
    case = Case("fake", "linear", "fake", lambda env: dict(ins={"x": torch.tensor([[1.0, 3e-13], [2.0, 1.0]])}, call=lambda T: called.append(1) or T["x"] * 1.0))
    tiny = Relation("rows", lambda ins, outs: ({"x": factors(2, 1)[:, None]}, [factors(2, 1)[:, None]]))
    with pytest.raises(AssertionError, match=rf"leave \[2\^-{MAG}, 2\^{MAG}\]"):       # 3e-13 in row 0 (x 2^20) is fine, in row 1 (x 2^-20) it is below 2^-60
        run_relation(Case("fake", "linear", "fake", lambda env: dict(ins={"x": torch.tensor([[1.0, 1.0], [2.0, 3e-13]])}, call=lambda T: called.append(1) or T["x"])), tiny)
    assert not called
    run_relation(case, tiny)
    # a factor that is no power of two, and a product that is not exact in the tensor's dtype
    with pytest.raises(AssertionError, match="powers of two"):
        scale_exact(torch.ones(2), torch.tensor([3.0, 1.0], dtype=torch.float64), "x")
    with pytest.raises(AssertionError, match="not exact"):
        scale_exact(torch.tensor([1e-38]), torch.tensor([2.0 ** -20], dtype=torch.float64), "x")          # into the subnormals
    # an output factor that overflows or flushes the baseline
    wide = Relation("rows", lambda ins, outs: ({"x": factors(2, 1)[:, None]}, [torch.full((2, 1), 2.0 ** 127, dtype=torch.float64)]))
    with pytest.raises(AssertionError, match="overflows"):
        run_relation(case, wide)
    # E8M0 exponent bytes: the product is a sum, and it must stay a valid byte
    assert scale_exact(torch.tensor([120, 130], dtype=torch.uint8), torch.tensor([4.0, 0.25], dtype=torch.float64), "sb").tolist() == [122, 128]
    with pytest.raises(AssertionError, match="leaves"):
        scale_exact(torch.tensor([1], dtype=torch.uint8), torch.tensor([0.5], dtype=torch.float64), "sb")


def test_mismatch_report_localises():
    want = torch.zeros(4, 5) + 1.0
    got = want.clone()
    got[2, 3] = torch.nextafter(torch.tensor(1.0), torch.tensor(2.0))
    got[2, 4] = 1.0 + 2.0 ** -21
    msg = describe_mismatch(got, want)
    assert "2 of 20 elements differ" in msg and "first at index (2, 3)" in msg and "largest difference 4 ulp" in msg
    assert "dim 0 (rows / samples): [2]" in msg and "dim 1 (columns / channels): [3, 4]" in msg


# ---- completeness --------------------------------------------------------------------------------------------------------------------------------------

def test_every_case_of_a_family_carries_a_relation_or_is_excluded_with_its_contract_line():
    cases = sg.all_cases()
    assert len(cases) > 400
    assert not set(sg.FAMILY_OF) & set(sg.OUT_OF_SCOPE)
    unknown = sorted({c.op for c in cases} - set(sg.FAMILY_OF) - set(sg.OUT_OF_SCOPE))
    assert not unknown, f"ops of the case tables that are neither in a family nor out of scope with a reason: {unknown}"
    stale = sorted((set(sg.FAMILY_OF) | set(sg.OUT_OF_SCOPE)) - {c.op for c in cases})
    assert not stale, f"ops no case table has: {stale}"
    by_name = {c.name: c for c in cases}
    for name, reason in sg.EXCLUDED.items():
        assert name in by_name, f"EXCLUDED names no case: {name}"
        # a reason quotes the absolute term of the op's contract and says where it stands
        assert re.search(r"\w+\.(h|hip|py)\b", reason) and re.search(r'"[^"]+"|`[^`]+`', reason), f"{name}: the reason cites no contract line: {reason!r}"
        assert "fail" not in reason.lower()
    missing = [c.name for c in cases if c.op in sg.FAMILY_OF and c.name not in sg.EXCLUDED and not sg.relations_for(c)]
    assert not missing, f"cases of a family without a relation: {missing}"
    # no kernel of a family is excluded wholesale: every op keeps cases that carry relations, on every kernel the tables name for it
    for op in sg.FAMILY_OF:
        mine = [c for c in cases if c.op == op]
        for kernel in {c.kernel for c in mine}:
            assert any(c.name not in sg.EXCLUDED for c in mine if c.kernel == kernel), f"{op} on {kernel}: every case is excluded"
    # the rows of the launch-configuration tables run under their own options: all of them belong to a family
    assert all(r.case.op in sg.FAMILY_OF for r in sg.LAUNCH_ROWS)
    assert all(r.name for c in cases for r in sg.relations_for(c))

"""The guard-band helper (tests/guard.py) on the CPU: fake ops that misbehave through the flat buffer, each in one way, must fail the
protocol, and the correct op must pass it -- otherwise tests/test_bounds_gpu.py would be vacuous.  And the completeness check: every
public callable of ``ops`` (and the optimizer's entry points) has a case in that file's table or a stated reason why it needs none."""
import inspect

import pytest
import torch

from tests import guard
from tests.guard import Case, check, guarded, run_case, run_fill

SHAPE = (5, 7)              # ragged: no multiple of any tile


def _is_guarded(t):
    """Does t live inside a guard-band buffer (storage with at least two guards around it)?  The fake ops step outside t only then."""
    return t.untyped_storage().nbytes() >= t.numel() * t.element_size() + 2 * guard.GUARD_MIN


def _at(t, offset, n=1):
    """n elements of t's storage starting ``offset`` elements from t's first one (outside t: only ever used on guarded views)."""
    assert _is_guarded(t)
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + offset)


def _double(x, out):
    return out.copy_(2 * x)


def _store_past_end(x, out):
    _double(x, out)
    if _is_guarded(out):
        _at(out, out.numel()).fill_(1.0)
    return out


def _store_before_start(x, out):
    _double(x, out)
    if _is_guarded(out):
        _at(out, -1).fill_(1.0)
    return out


def _skips_an_element(x, out):
    flat, src = out.view(-1), (2 * x).view(-1)
    flat[:17].copy_(src[:17])
    flat[18:].copy_(src[18:])
    return out


def _modifies_input(x, out):
    _double(x, out)
    x[1, 1] += 1.0
    return out


def _zero_mask_instead_of_select(x, out):
    stray = _at(x, x.numel())[0] if _is_guarded(x) else 0.0
    return out.copy_(2 * x + 0.0 * stray)


def _row_past_end(x, out):
    _double(x, out)
    if _is_guarded(out):
        _at(out, out.numel(), SHAPE[1]).copy_(2 * x[-1])
    return out


def _case(fn, name):
    def make(env):
        x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(1))
        return dict(ins={"x": x}, outs={"y": (SHAPE, torch.float32)}, call=lambda T: fn(T["x"], T["y"]), ref=lambda R: 2 * R["x"], tol=1e-6)
    return Case(name, "double", "fake", make)


def test_correct_op_passes():
    res = run_case(_case(_double, "double"), "nan")
    assert len(res.outputs) == 1 and res.errs[0] < 1e-6


@pytest.mark.parametrize("fn,what", [(_store_past_end, "PAST the tensor's end, first at byte offset 140"),
                                     (_store_before_start, "BEFORE the tensor, first at byte offset -4"),
                                     (_skips_an_element, "never written (still NaN), first at flat index 17"),
                                     (_modifies_input, "input modified, 4 byte(s), first at byte offset 32"),
                                     (_row_past_end, "28 byte(s) written PAST the tensor's end, first at byte offset 140")])
def test_misbehaviour_is_caught(fn, what):
    for fill in guard.FILLS:
        with pytest.raises(AssertionError, match=what.replace("(", r"\(").replace(")", r"\)")):
            run_case(_case(fn, fn.__name__), fill)


def test_dependence_on_out_of_bounds_data_is_caught():
    """value + 0 * (element past the end): right under finite strays (the FLT_MAX fill alone passes, as a test on allocator memory does),
    caught by the NaN fill and by the comparison of the two fills."""
    case = _case(_zero_mask_instead_of_select, "zero_mask")
    run_fill(case, "big")
    with pytest.raises(AssertionError):
        run_fill(case, "nan")
    for fill in guard.FILLS:
        with pytest.raises(AssertionError):
            run_case(case, fill)
    a, b = (_zero_mask_instead_of_select(guarded(torch.ones(SHAPE), fill)[0], torch.empty(SHAPE)) for fill in guard.FILLS)
    assert not guard.same_bits(a, b)             # what check 3 compares


def test_ignored_out_argument_is_caught():
    def fresh(x, out):
        return 2 * x
    with pytest.raises(AssertionError, match="never written"):
        run_fill(_case(fresh, "ignores_out"), "nan")


def test_inplace_operand_is_exempt_from_the_payload_rule_only():
    def make_ok(env):
        x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(2))
        return dict(ins={"x": x}, call=lambda T: T["x"].mul_(2), ref=lambda R: 2 * R["x"], tol=1e-6, inplace=("x",))
    run_case(Case("inplace", "double_", "fake", make_ok), "nan")

    def bad(x):
        x.mul_(2)
        if _is_guarded(x):
            _at(x, x.numel()).fill_(0.0)
        return x

    def make_bad(env):
        return dict(make_ok(env), call=lambda T: bad(T["x"]))
    with pytest.raises(AssertionError, match="PAST"):
        run_case(Case("inplace_overshoot", "double_", "fake", make_bad), "big")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int64, torch.int32])
@pytest.mark.parametrize("shape", [(), (1,), (5, 7), (3, 300), (2, 3, 129)])
def test_layout_and_fills(dtype, shape):
    t = (torch.arange(max(1, int(torch.tensor(shape).prod())) if shape else 1) % 100).reshape(shape).to(dtype)
    for fill in guard.FILLS:
        v, h = guarded(t, fill)
        assert v.shape == t.shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 256 == 0 and torch.equal(v, t)
        gb = h.guard
        assert gb >= 64 * 1024 and gb >= 256 * (t.shape[-1] if t.dim() else 1) * t.element_size() and gb % 256 == 0
        lowg = h.buf[h.lo - gb:h.lo].view(dtype)
        highg = h.buf[h.lo + h.nbytes + (-h.nbytes) % 256 or 256 * (h.nbytes == 0):][:gb].view(dtype)
        for gd in (lowg, highg):
            if dtype.is_floating_point:
                assert bool(torch.isnan(gd).all()) if fill == "nan" else bool((gd == torch.finfo(dtype).max).all())
            elif dtype == torch.uint8:
                assert bool((gd == (0xFF if fill == "nan" else 0x7F)).all())
            else:
                assert bool((gd == (torch.iinfo(dtype).min if fill == "nan" else torch.iinfo(dtype).max)).all())
        check(h)
    v, h = guarded(t, "out")
    assert bool((h.buf[:h.lo] == 0xA5).all()) and bool((h.buf[h.lo + h.nbytes:] == 0xA5).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(v).all())
    check(h)
    h.buf[h.lo - 1] = 0
    with pytest.raises(AssertionError, match="BEFORE"):
        check(h)


# ---- completeness: every op has a case ------------------------------------------------------------------------------------------------

EXEMPT = {
    "pack_weight": "host cache around the pack kernels; every split3 / bf16 / mx8 GEMM and ffn case goes through it",
    "ffn_supported": "predicate, no launch",
    "attn_ffn_supported": "predicate, no launch",
    "wgrad_chunks": "host arithmetic, no launch",
    "wgrad_chunks_bf16": "host arithmetic, no launch",
    "jacobi_tol": "host arithmetic, no launch",
    "rk_error_sq": "host sum of rk_error_partial's result, which has its case",
}


def test_every_op_has_a_case_or_a_reason():
    import k_diffusion_amd as KD
    from tests import test_bounds_gpu as tb
    ops = KD.ops
    public = sorted(n for n, f in vars(ops).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == ops.__name__)
    public += ["AdamW.step", "ema_update"]
    assert callable(KD.optim.AdamW.step) and callable(KD.optim.ema_update)
    covered = {c.op for c in tb.CASES}
    assert not covered & set(EXEMPT), covered & set(EXEMPT)
    missing = [n for n in public if n not in covered and n not in EXEMPT]
    assert not missing, f"no guard-band case and no stated exemption: {missing}"
    unknown = sorted((covered | set(EXEMPT)) - set(public))
    assert not unknown, f"cases / exemptions for callables that do not exist: {unknown}"
    names = [c.name for c in tb.CASES]
    assert len(names) == len(set(names)), "case names are the test ids: unique"
    for c in tb.CASES:
        assert c.src.endswith((".hip", ".py")) and c.mode in (None, "exact", "split3", "bf16"), c.name

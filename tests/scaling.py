"""Power-of-two scaling relations: a kernel that is linear in an operand must commute with scaling that operand by powers of two, bit for bit.

Multiplying by 2^k is exact in fp32, in bf16 and in the hi / lo bf16 split (``bf16(x)`` and ``bf16(x - hi)`` both scale exactly), and it stays
exact through an fp32 or fp64 accumulation in a fixed order.  So no tolerance appears anywhere in this file: a relation holds in every bit or
it does not hold.  With exponents spread over +-20 between neighbouring rows, samples or channels, a trace of 1e-6 of one row in the next one,
or any absolute constant in the arithmetic, changes bits.

A **relation** (``Relation``) is a named function of a case's ``ins`` (tests/guard.py: ``case.make(env)``) returning

* ``in_factors``: {input name: tensor of powers of two, broadcastable to that input}; inputs not named are unscaled.  A uint8 input that is
  named holds E8M0 exponent bytes: its "product" is the byte plus log2 of the factor;
* ``out_factors``: one factor tensor per result (None: the same bits as the baseline), or a function of the baseline results returning that list.

``run_relation`` runs the case's ``call`` on the plain inputs (the baseline) and on the scaled ones and asserts that every result has the bits of
``baseline * out_factor``.  The products are formed on the CPU in the tensor's own dtype and checked there to be exact (``x * f / f == x`` bitwise).
Before anything runs it asserts that every scaled floating input has its nonzero magnitudes inside [2^-60, 2^60] and that ``baseline * out_factor``
has no new zero and no inf: no relation may depend on what the hardware does with subnormals, and with exponents in [-20, 20] applied one relation
at a time every product -- and every ``lo`` part of a split operand, 2^-8 below its ``hi`` -- stays far from that range.

Plain Python on any device: tests/test_scaling_cpu.py seeds each kind of defect with fake ops on the CPU and shows which relation catches it.
"""
import torch

LIM = 20                    # exponents of the factors: integers in [-LIM, LIM]
LIM_E8M0 = 8                # for operands behind a power-of-two block or channel scale (fp8 products)
MAG = 60                    # every scaled floating input: nonzero magnitudes in [2^-MAG, 2^MAG]

_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float64: torch.int64}


def exponents(n, seed, lim=LIM):
    """n integers in [-lim, lim] from a seeded generator; index 0 is +lim and index 1 is -lim, so the two extremes are neighbours."""
    k = torch.randint(-lim, lim + 1, (n,), generator=torch.Generator().manual_seed(1000003 * seed + n))
    if n >= 1:
        k[0] = lim
    if n >= 2:
        k[1] = -lim
    return k


def pow2(k):
    return torch.ldexp(torch.ones(k.shape, dtype=torch.float64), k)


def factors(n, seed, lim=LIM):
    """[n] float64 powers of two with exponents ``exponents(n, seed, lim)``"""
    return pow2(exponents(n, seed, lim))


def along(f, ndim, dim):
    """the 1-D factor ``f`` shaped to broadcast along ``dim`` of an ``ndim``-dimensional tensor"""
    shape = [1] * ndim
    shape[dim] = f.numel()
    return f.reshape(shape)


class Relation:
    """``fn(ins, outs) -> (in_factors, out_factors)`` (``outs``: the case's {name: (shape, dtype)} of its ``out=`` operands).  ``zero``: inputs
    replaced by zeros in BOTH calls (a bias, where the relation is stated without one).  ``views``: {input name: dtype} -- the factor applies to
    the input viewed as that dtype (bf16 pairs stored in fp32 words)."""

    def __init__(self, name, fn, zero=(), views=None):
        self.name, self.fn, self.zero, self.views = name, fn, tuple(zero), dict(views or {})

    def __repr__(self):
        return self.name


def _bits(t):
    return t.contiguous().view(_INT[t.dtype]) if t.dtype in _INT else t.contiguous()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _log2(f):
    k = torch.log2(f.double())
    assert torch.equal(k, k.round()), "factors must be powers of two"
    return k.to(torch.int64)


def scale_exact(x, f, what):
    """``x * f`` in x's own dtype, asserted exact; for uint8 (E8M0 exponent bytes) the byte plus log2 f, asserted inside [1, 254]."""
    _log2(f)
    if x.dtype == torch.uint8:
        y = x.to(torch.int64) + _log2(f)
        assert int(y.min()) >= 1 and int(y.max()) <= 254, f"{what}: an exponent byte leaves [1, 254]"
        return y.to(torch.uint8)
    assert x.is_floating_point(), f"{what}: {x.dtype} cannot be scaled"
    fx = f.to(x.dtype)
    assert torch.equal(fx.double(), f.double()), f"{what}: a factor is not exact in {x.dtype}"
    y = x * fx
    assert same_bits(y / fx, x.expand_as(y).contiguous()), f"{what}: the product with the factors is not exact"
    nz = y[y != 0].abs().double()
    if nz.numel():
        assert float(nz.min()) >= 2.0 ** -MAG and float(nz.max()) <= 2.0 ** MAG, (f"{what}: scaled magnitudes [{float(nz.min()):.3e}, {float(nz.max()):.3e}] "
                                                                                  f"leave [2^-{MAG}, 2^{MAG}]")
    return y


def expected(base, f, what):
    """``base * f`` for a result (None: base itself), with the conditions on it: no zero that was nonzero in the baseline, no inf."""
    if f is None:
        return base
    if base.dtype == torch.uint8:
        return scale_exact(base, f, what)
    fx = f.to(base.dtype)
    assert torch.equal(fx.double(), _pow2_check(f)), f"{what}: a factor is not exact in {base.dtype}"
    want = base * fx
    assert want.shape == base.shape, f"{what}: the factor {tuple(f.shape)} does not broadcast to the result {tuple(base.shape)}"
    assert not bool(torch.isinf(want).any()), f"{what}: baseline * factor overflows"
    assert not bool(((want == 0) & (base != 0)).any()), f"{what}: baseline * factor flushes a nonzero result to zero"
    assert same_bits(want / fx, base), f"{what}: baseline * factor is not exact"
    return want


def _pow2_check(f):
    _log2(f)
    return f.double()


def _ordered(t):
    """the bit pattern of a floating tensor as integers that order like the values (for distances in ulps)"""
    i = _bits(t).to(torch.int64)
    if t.dtype == torch.float64:
        return torch.where(i < 0, -(i & (2 ** 63 - 1)), i).double()
    sign = 1 << (8 * t.element_size() - 1)
    return torch.where(i < 0, -(i & (sign - 1)), i)


def _some(idx, limit=12):
    idx = sorted(set(int(i) for i in idx))
    return f"{idx[:limit]}{' ... (%d in all)' % len(idx) if len(idx) > limit else ''}"


def describe_mismatch(got, want):
    """How two tensors of the same shape and dtype differ: count, first index, largest distance in ulps, and along every dimension the indices
    the differing elements fall in (dimension 0: rows or samples, the last one: columns or channels) -- what localises a leak."""
    ne = (_bits(got) != _bits(want)).reshape(got.shape)
    where = ne.nonzero()
    n = int(where.shape[0])
    if got.is_floating_point():
        ulps = (_ordered(got) - _ordered(want)).abs().max().item()
        nonfinite = int((~torch.isfinite(got)).sum())
    else:
        ulps, nonfinite = (got.to(torch.int64) - want.to(torch.int64)).abs().max().item(), 0
    dims = "; ".join(f"dim {d} ({'rows / samples' if d == 0 and got.dim() > 1 else 'columns / channels' if d == got.dim() - 1 else 'axis'}): {_some(where[:, d])}"
                     for d in range(got.dim()))
    return (f"{n} of {got.numel()} elements differ, first at index {tuple(int(i) for i in where[0])} (got {got[tuple(where[0])].item()!r}, "
            f"want {want[tuple(where[0])].item()!r}), largest difference {ulps:.0f} ulp{', %d non-finite' % nonfinite if nonfinite else ''}; {dims}")


def _as_tuple(x):
    return (x,) if isinstance(x, torch.Tensor) else tuple(x)


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def run_call(spec, ins, device):
    """The case's ``call`` on ``ins`` (CPU tensors) with fresh ``out=`` operands -> its results on the CPU."""
    T = {k: v.to(device).clone() for k, v in ins.items()}
    T.update({k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in spec.get("outs", {}).items()})
    got = [t.detach().cpu().clone() for t in _as_tuple(spec["call"](T))]
    _sync(device)
    return got


def plain_inputs(spec, relation):
    ins = dict(spec["ins"])
    for k in relation.zero:
        ins[k] = torch.zeros_like(ins[k])
    return ins


def scaled_inputs(case, relation, ins, outs):
    """(the scaled inputs, out_factors) of ``relation`` on ``ins``; every product formed on the CPU and checked exact."""
    in_factors, out_factors = relation.fn(ins, outs)
    assert in_factors, f"{case.name} / {relation.name}: no input is scaled"
    scaled = dict(ins)
    for k, f in in_factors.items():
        what = f"{case.name} / {relation.name}: input {k!r}"
        x = ins[k]
        if k in relation.views:
            scaled[k] = scale_exact(x.contiguous().view(relation.views[k]), f, what).view(x.dtype).view(x.shape)
        else:
            scaled[k] = scale_exact(x, f, what)
        assert scaled[k].shape == x.shape, f"{what}: the factor {tuple(f.shape)} does not broadcast to {tuple(x.shape)}"
        assert not same_bits(scaled[k], x.contiguous()), f"{what}: the factors change nothing"
    return scaled, out_factors


def run_relation(case, relation, env=None, device="cpu", spec=None, baseline=None, on_call=None):
    """One relation on one case.  ``spec`` / ``baseline``: ``case.make(env)`` and the results of the plain call from an earlier relation of the
    same case with the same ``zero`` (computed once, shared).  ``on_call(which)``: called after each call ("baseline" / "scaled"), for the
    launch profile.  Returns (spec, baseline)."""
    spec = spec if spec is not None else case.make(env)
    ins = plain_inputs(spec, relation)
    scaled, out_factors = scaled_inputs(case, relation, ins, spec.get("outs", {}))
    if baseline is None:
        baseline = run_call(spec, ins, device)
        if on_call:
            on_call("baseline")
    if callable(out_factors):
        out_factors = out_factors(baseline)
    assert len(out_factors) == len(baseline), f"{case.name} / {relation.name}: {len(baseline)} results, {len(out_factors)} output factors"
    want = [expected(b, f, f"{case.name} / {relation.name}: result {i}") for i, (b, f) in enumerate(zip(baseline, out_factors))]
    got = run_call(spec, scaled, device)
    if on_call:
        on_call("scaled")
    for i, (g, w, f) in enumerate(zip(got, want, out_factors)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{case.name} / {relation.name}: result {i} changed shape or dtype"
        if not same_bits(g, w):
            raise AssertionError(f"{case.name} / {relation.name}: result {i} is not the baseline {'unchanged' if f is None else 'times its factors'}: "
                                 f"{describe_mismatch(g, w)}")
    return spec, baseline

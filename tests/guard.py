"""Guard bands around the tensors a kernel is handed: does it read or write outside them, and does it write everything inside?

``guarded(t, fill)`` lays ``[low guard | payload | high guard]`` out in ONE flat uint8 allocation and returns a contiguous, 256-byte
aligned view of the payload with ``t``'s shape and dtype -- to the op it looks like any other allocation -- plus a handle.  An overshoot
of up to a tile therefore lands in memory the process owns and shows up in ``check(handle)`` as a changed byte, never as a fault.

Inputs get their guards filled with "nan" (quiet NaN of the dtype; 0xFF for uint8; INT_MIN for integer ids) or with "big" (the largest
finite value; 0x7F for uint8; INT_MAX for integer ids -- out of range for every index tensor in both fills).  A kernel that loads out of
range and multiplies by a zero mask instead of selecting gives different bits under the two fills.  Outputs get 0xA5 guards and a NaN
payload: every reference here is finite, so a NaN left in an output is an element the kernel never wrote.

``run_fill(case, fill, env)`` runs the checks of one fill (reference, same bits as the ordinary call, guards and inputs intact,
everything written); ``run_case(case, fill, env)`` is the whole protocol: that fill, the other one, and the comparison between them.  Plain Python on any device:
tests/test_guard_cpu.py seeds each kind of misbehaviour with fake ops on the CPU and shows that the protocol catches it.
"""
import torch

from tests.helpers import relerr

ALIGN = 256                 # payload address and guard sizes are multiples of this
GUARD_MIN = 64 * 1024       # bytes
GUARD_ROWS = 256            # rows of the tensor's last dimension: one full tile of overshoot for any kernel here
OUT_GUARD_BYTE = 0xA5

# dtype -> (integer dtype of the same width, bit pattern)
_NAN = {torch.float32: (torch.int32, 0x7FC00000), torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00),
        torch.float64: (torch.int64, 0x7FF8000000000000), torch.uint8: (torch.uint8, 0xFF),
        torch.int32: (torch.int32, -2 ** 31), torch.int64: (torch.int64, -2 ** 63)}
_BIG = {torch.float32: (torch.int32, 0x7F7FFFFF), torch.bfloat16: (torch.int16, 0x7F7F), torch.float16: (torch.int16, 0x7BFF),
        torch.float64: (torch.int64, 0x7FEFFFFFFFFFFFFF), torch.uint8: (torch.uint8, 0x7F),
        torch.int32: (torch.int32, 2 ** 31 - 1), torch.int64: (torch.int64, 2 ** 63 - 1)}
FILLS = ("nan", "big")


def _round_up(n, m):
    return -(-n // m) * m


def guard_bytes(t):
    """Size of each guard of ``t``: at least 64 KiB and at least 256 rows of its last dimension, rounded up to 256 bytes."""
    row = (t.shape[-1] if t.dim() else 1) * t.element_size()
    return _round_up(max(GUARD_MIN, GUARD_ROWS * row), ALIGN)


def _fill_pattern(region, dtype, table):
    idt, pat = table[dtype]
    region.view(idt).fill_(pat)


class Handle:
    """One guarded tensor: the flat buffer, where the payload lies in it, and the bytes it held when it was handed out."""

    def __init__(self, buf, lo, nbytes, guard, kind, name):
        self.buf, self.lo, self.nbytes, self.guard, self.kind, self.name = buf, lo, nbytes, guard, kind, name
        self.before = buf.clone()


def guarded(t, fill, name=""):
    """(view, handle).  ``fill``: "nan" / "big" for an input (the payload is a copy of ``t``), "out" for an output (0xA5 guards, NaN
    payload; only ``t``'s shape, dtype and device are used)."""
    if fill not in FILLS + ("out",):
        raise ValueError(f"fill {fill!r}: one of 'nan', 'big', 'out'")
    if t.dtype not in _NAN:
        raise TypeError(f"guarded: no fill patterns for {t.dtype}")
    nbytes = t.numel() * t.element_size()
    gb = guard_bytes(t)
    payload_room = _round_up(max(nbytes, 1), ALIGN)        # the high guard starts on a 256-byte boundary at or after the payload's end
    buf = torch.empty(gb + payload_room + gb + ALIGN, dtype=torch.uint8, device=t.device)
    lo = (-buf.data_ptr()) % ALIGN + gb                    # byte offset of the payload: 256-byte aligned address, >= one guard in front
    if fill == "out":
        buf.fill_(OUT_GUARD_BYTE)
        if nbytes:
            _fill_pattern(buf[lo:lo + nbytes], t.dtype, _NAN)
    else:
        table = _NAN if fill == "nan" else _BIG
        _fill_pattern(buf[lo - gb:lo + payload_room + gb], t.dtype, table)
        head = (lo - gb)
        buf[:head].fill_(OUT_GUARD_BYTE)
        buf[lo + payload_room + gb:].fill_(OUT_GUARD_BYTE)
    view = buf[lo:lo + nbytes].view(t.dtype).view(t.shape)
    if fill != "out" and nbytes:
        view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % ALIGN == 0 and view.shape == t.shape
    return view, Handle(buf, lo, nbytes, gb, "out" if fill == "out" else "in", name)


def _first_diff(a, b):
    ne = (a != b).nonzero()
    return int(ne[0]), int(ne.numel())


def check(handle, payload=None):
    """Guards bytewise unchanged; for an input (or with ``payload=True``) the payload too.  Raises AssertionError naming the first
    changed byte relative to the payload (negative: before its start; >= its size: past its end)."""
    h = handle
    now, was = h.buf, h.before
    end = h.lo + h.nbytes
    if not torch.equal(now[:h.lo], was[:h.lo]):
        at, n = _first_diff(now[:h.lo], was[:h.lo])
        raise AssertionError(f"{h.name}: {n} byte(s) written BEFORE the tensor, first at byte offset {at - h.lo} (payload of {h.nbytes} bytes)")
    if not torch.equal(now[end:], was[end:]):
        at, n = _first_diff(now[end:], was[end:])
        raise AssertionError(f"{h.name}: {n} byte(s) written PAST the tensor's end, first at byte offset {h.nbytes + at} (payload of {h.nbytes} bytes)")
    if (h.kind == "in") if payload is None else payload:
        if not torch.equal(now[h.lo:end], was[h.lo:end]):
            at, n = _first_diff(now[h.lo:end], was[h.lo:end])
            raise AssertionError(f"{h.name}: input modified, {n} byte(s), first at byte offset {at}")


def _as_tuple(x):
    if isinstance(x, torch.Tensor):
        return (x,)
    return tuple(t if isinstance(t, torch.Tensor) or t is None else torch.tensor(t, dtype=torch.float64) for t in (x if isinstance(x, (tuple, list)) else (x,)))


def _bytes(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def compare(got, ref, tol):
    """One output against its reference.  ``tol``: 0 -- bit for bit (``ref`` in the output's dtype); a float -- tests.helpers.relerr
    (max norm); ("abs", x) -- largest absolute difference (the existing test of that op states its bound that way); a callable
    (got, ref) -> error that asserts a rule of its own (the optimizer's fp32-yardstick rule)."""
    if callable(tol):
        return tol(got, ref)
    if tol == 0:
        ref = ref.to(got.dtype)
        assert same_bits(got.cpu().reshape(ref.shape), ref), f"not bit-identical with the reference ({int((got.cpu().reshape(ref.shape) != ref).sum())} elements differ)"
        return 0.0
    g64, r64 = got.detach().cpu().double().reshape(ref.shape), ref.detach().cpu().double()
    if isinstance(tol, tuple):
        kind, bound = tol
        assert kind == "abs"
        err = (g64 - r64).abs().max().item() if r64.numel() else 0.0
    else:
        bound = tol
        err = relerr(g64, r64) if r64.numel() else 0.0
    assert err < bound, f"error {err:.3e} against the reference, bound {bound:.1e}"
    return err


class Result:
    def __init__(self, outputs, refs, errs):
        self.outputs, self.refs, self.errs = outputs, refs, errs


def _ref_inputs(ins, ref32):
    return {k: (v.clone() if ref32 or not v.is_floating_point() else v.double()) for k, v in ins.items()}


def run_fill(case, fill, env=None, device="cpu", refs=None):
    """Checks 1, 2, 4 and 5 of the protocol for ``case`` under one fill; returns a Result (outputs on the CPU, references, errors).

    ``case.make(env)`` returns a dict: ``ins`` {name: CPU tensor}; ``outs`` {name: (shape, dtype)} for the ``out=`` operands (may be
    empty: the op allocates its results, and only its inputs are guarded); ``call(T)`` running the op on the dict T of device tensors
    and returning its result tensor(s); ``ref(R)`` the reference on the CPU from R (floating inputs in float64, or as they are with
    ``ref32``: the oracle's fp32 functions in the kernel's rounding order, for bit-exact ops); ``tol`` one bound or a list of one per
    result (None: that result has no reference of its own and only takes part in the bit and NaN checks); ``inplace``: names of inputs the op documents as rewritten (exempt from the untouched-payload rule).  ``refs``: the references
    of an earlier run of the same case (computed once, shared)."""
    spec = case.make(env)
    ins, outs = spec["ins"], spec.get("outs", {})
    inplace = set(spec.get("inplace", ()))
    tols = spec["tol"]
    # the ordinary call: plain tensors from the allocator
    T = {k: v.to(device).clone() for k, v in ins.items()}
    T.update({k: torch.empty(shape, dtype=dt, device=device) for k, (shape, dt) in outs.items()})
    plain = [t.detach().clone() for t in _as_tuple(spec["call"](T))]
    # the guarded call
    G, handles = {}, {}
    for k, v in ins.items():
        G[k], handles[k] = guarded(v.to(device), fill, f"{case.name}: input {k!r}")
    for k, (shape, dt) in outs.items():
        G[k], handles[k] = guarded(torch.empty(shape, dtype=dt, device=device), "out", f"{case.name}: output {k!r}")
    got = _as_tuple(spec["call"](G))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    # 4. nothing outside is touched, inputs are not modified
    for k, h in handles.items():
        check(h, payload=False if k in inplace else None)
    # 5. everything inside is written: the guarded outputs themselves (an op that ignored ``out=`` leaves the pre-fill there) ...
    for k in outs:
        h, o = handles[k], G[k]
        if o.is_floating_point():
            left = int(torch.isnan(o).sum())
            assert left == 0, f"{h.name}: {left} of {o.numel()} elements never written (still NaN), first at flat index {int(torch.isnan(o).reshape(-1).nonzero()[0])}"
        elif h.nbytes:
            assert not torch.equal(h.buf[h.lo:h.lo + h.nbytes], h.before[h.lo:h.lo + h.nbytes]), f"{h.name}: the output still holds its pre-fill: never written"
    # ... and what the op returned
    for i, o in enumerate(got):
        if o.is_floating_point():
            left = int(torch.isnan(o).sum())
            assert left == 0, f"{case.name}: result {i}: {left} of {o.numel()} elements never written (still NaN), first at flat index {int(torch.isnan(o).reshape(-1).nonzero()[0])}"
    # 2. the same bits as the ordinary call
    assert len(got) == len(plain)
    for i, (a, b) in enumerate(zip(got, plain)):
        assert same_bits(a, b), f"{case.name}: result {i}: the guarded call differs from the ordinary call on the same values"
    # 1. the reference
    if refs is None:
        refs = _as_tuple(spec["ref"](_ref_inputs(ins, spec.get("ref32", False))))
    assert len(refs) == len(got), f"{case.name}: {len(got)} results, {len(refs)} references"
    if not isinstance(tols, list):
        tols = [tols] * len(got)
    errs = []
    for i, (a, r, tol) in enumerate(zip(got, refs, tols)):
        if tol is None:
            errs.append(0.0)
            continue
        try:
            errs.append(compare(a, r, tol))
        except AssertionError as e:
            raise AssertionError(f"{case.name}: result {i}: {e}") from None
    return Result([o.detach().cpu().clone() for o in got], refs, errs)


def run_case(case, fill, env=None, device="cpu"):
    """The whole protocol for one case: checks 1, 2, 4 and 5 under ``fill`` (``run_fill``), the same under the other fill with the
    references shared, and check 3 -- the results of the two are the same bits, so nothing outside the inputs entered them.  Returns the
    Result of the run under ``fill``."""
    other = FILLS[1 - FILLS.index(fill)]
    a = run_fill(case, fill, env, device)
    b = run_fill(case, other, env, device, refs=a.refs)
    for i, (x, y) in enumerate(zip(a.outputs, b.outputs)):
        assert same_bits(x, y), (f"{case.name}: result {i} depends on memory outside its inputs: {int((_bytes(x) != _bytes(y)).sum())} bytes differ "
                                 f"between the NaN-filled and the FLT_MAX-filled guards")
    return a


class Case:
    """One row of a case table: one launch path of one op at one shape.  ``op``: the public callable it covers (the completeness check
    reads it); ``src``: the source file of the kernel; ``mode``: the arithmetic mode it runs under ("exact" / "split3" / None for ops that
    ignore it); ``few_rows``: runs with the few-rows kernels at their defaults; ``kernel``: prefix of the launch-profile name that must
    have served it; ``make``: see ``run_fill``."""

    def __init__(self, name, op, src, make, mode=None, few_rows=False, kernel=None):
        self.name, self.op, self.src, self.make, self.mode, self.few_rows, self.kernel = name, op, src, make, mode, few_rows, kernel

    def __repr__(self):
        return self.name

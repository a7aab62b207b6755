"""The derivative plumbing of k_diffusion_amd.compat without a GPU: the ``ops`` functions compat calls are replaced by fakes that evaluate
the CPU oracle (forward, reverse mode and forward mode, in fp64, returned in fp32), so what is checked is what compat itself adds around a
kernel -- the operators' layouts, the packing of primals and tangents, the softmax scale folded into q and carried back onto its gradient,
which tensor is saved, and the import shims.  The kernels themselves are checked on the device (tests/test_compat_grad_gpu.py, which also
takes the operator table below from here)."""
import functools
from types import SimpleNamespace

import pytest
import torch
from torch.autograd import forward_ad

from oracle import hdit

N, NH, E = 2, 3, 64                 # three heads: a head stride that is no power of two
DEFAULT_SCALE = E ** -0.5           # what natten, flash-attn and SDPA use when no scale is given


# ---- the operators in the reference's own layouts ---------------------------------------------------------------------------------------------
# Each entry: ``views(proj)`` cuts the operator's inputs out of one projection output [n, h, w, 3 * nh * 64] the way the reference's block
# does (strided views, not copies); ``call(C, ins, scale)`` is the compat call; ``ref(ins, scale)`` the oracle in the same layout.

def operator(name, arg, H, W):
    s = H * W
    eff = lambda scale: DEFAULT_SCALE if scale is None else scale
    if name == "na2d":                                      # "n h w (t nh e) -> t n h w nh e"
        return SimpleNamespace(
            views=lambda p: p.view(N, H, W, 3, NH, E).unbind(3),
            call=lambda C, ins, scale: C.na2d(*ins, arg) if scale is None else C.na2d(*ins, kernel_size=arg, scale=scale),
            ref=lambda ins, scale: hdit.na2d(*ins, arg, eff(scale)))
    if name == "flash":                                     # "n h w (t nh e) -> n (h w) t nh e": one packed input
        return SimpleNamespace(
            views=lambda p: (p.view(N, s, 3, NH, E),),
            call=lambda C, ins, scale: C.flash_attn_qkvpacked_func(ins[0], softmax_scale=scale),
            ref=lambda ins, scale: hdit.attn_global(*(t.reshape(N, H, W, NH, E) for t in ins[0].unbind(2)), eff(scale)).reshape(N, s, NH, E))
    if name == "sdpa":                                      # "n h w (t nh e) -> t n nh (h w) e"
        return SimpleNamespace(
            views=lambda p: p.view(N, s, 3, NH, E).permute(2, 0, 3, 1, 4).unbind(0),
            call=lambda C, ins, scale: C.scaled_dot_product_attention(*ins, scale=scale),
            ref=lambda ins, scale: hdit.attn_global(*(t.transpose(1, 2).reshape(N, H, W, NH, E) for t in ins), eff(scale))
            .reshape(N, s, NH, E).transpose(1, 2))
    assert name == "window"                                 # "n h w (t nh e) -> t n nh h w e"
    return SimpleNamespace(
        views=lambda p: p.view(N, H, W, 3, NH, E).permute(3, 0, 4, 1, 2, 5).unbind(0),
        call=lambda C, ins, scale: C.apply_window_attention(*arg, *ins, scale=scale),
        ref=lambda ins, scale: hdit.attn_shifted_window(*(t.permute(0, 2, 3, 1, 4) for t in ins), *arg, eff(scale)).permute(0, 3, 1, 2, 4))


def projection(H, W, seed):
    """[n, h, w, 3 * nh * 64] fp32: q and k unit rows times sqrt(10) (the cosine-sim scale), v normal."""
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(N, H, W, NH, E, generator=gen) for _ in range(3))
    q, k = hdit.cosine_sim_scale(q, k, torch.full([NH], 10.0))
    return torch.cat([q.flatten(-2), k.flatten(-2), v.flatten(-2)], dim=-1)


def slots(ins):
    """The q, k and v parts of an operator's inputs (or of their gradients / tangents): the packed operator has them in one tensor."""
    return ins[0].unbind(2) if len(ins) == 1 else ins


def like_inputs(op, H, W, seed, dtype=torch.float32):
    """Random tensors shaped like the operator's inputs (tangents) and one shaped like its output (the gradient handed to backward)."""
    gen = torch.Generator().manual_seed(seed)
    ins = op.views(torch.zeros(N, H, W, 3 * NH * E))
    tangents = tuple(torch.randn(t.shape, generator=gen).to(dtype) for t in ins)
    shape = slots(ins)[0].shape
    return tangents, torch.randn(shape, generator=gen).to(dtype)


@functools.lru_cache(maxsize=None)
def reference(name, arg, H, W, scale, seed, dtype):
    """fp64 reverse-mode autograd of the oracle at inputs rounded to ``dtype``, computed once per case and shared: the projection, the
    gradient handed to backward, tangents, the output and the gradients per input.  Nothing of it is modified by a test."""
    op = operator(name, arg, H, W)
    proj = projection(H, W, seed).to(dtype)
    tangents, g_out = like_inputs(op, H, W, seed + 1, dtype)
    ins = op.views(proj.double().requires_grad_())
    with torch.enable_grad():
        out = op.ref(ins, scale)
        grads = torch.autograd.grad(out, ins, g_out.double())
    return SimpleNamespace(op=op, scale=scale, proj=proj, g_out=g_out, tangents=tangents, out=out.detach(), grads=grads)


@functools.lru_cache(maxsize=None)
def reference_jvp(name, arg, H, W, scale, seed, dtype):
    """fp64 ``torch.autograd.functional.jvp`` of the oracle for the same case: o_dot for the tangents on every input, and for v's alone."""
    r = reference(name, arg, H, W, scale, seed, dtype)
    f = lambda *a: r.op.ref(a, scale)
    ins = tuple(t.double() for t in r.op.views(r.proj))
    return tuple(torch.autograd.functional.jvp(f, ins, tuple(t.double() for t in tg))[1] for tg in (r.tangents, v_only(r.tangents)))


def v_only(tangents):
    """The same tangents with the q and k parts zeroed."""
    if len(tangents) == 1:
        t = tangents[0].clone()
        t[:, :, :2] = 0
        return (t,)
    return (torch.zeros_like(tangents[0]), torch.zeros_like(tangents[1]), tangents[2])


def attention_node(out):
    """The ``_Attention`` node of the graph behind ``out`` (the operators add views after it)."""
    todo = [out.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None:
            continue
        if "_Attention" in type(fn).__name__:
            return fn
        todo += [f for f, _ in fn.next_functions]
    raise AssertionError("no _Attention node in the graph")


def relerr64(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


# ---- oracle-backed fakes of the ops compat calls ----------------------------------------------------------------------------------------------

def _packed_oracle(kind):
    def f(x, nh, *arg):
        x4 = x if x.dim() == 4 else x.reshape(x.shape[0], 1, -1, x.shape[-1])
        q, k, v = hdit.split_qkv(x4, nh)
        o = {"na2d": hdit.na2d, "window": hdit.attn_shifted_window, "global": hdit.attn_global}[kind](q, k, v, *arg)
        return o.reshape(*x.shape[:-1], nh * E)
    return f


@pytest.fixture
def fake(monkeypatch):
    """compat on CPU tensors: ops.attn_* / _vjp / _jvp evaluate the oracle in fp64, the device check is off, and fp32 tensors take the
    plain-operand path.  Returns the package and the list of (kind, qkv, g_out) that reached the fake VJPs."""
    import k_diffusion_amd as KD
    seen = []
    for kind in ("na2d", "window", "global"):
        f = _packed_oracle(kind)

        def fwd(qkv, nh, *arg, prep=None, out=None, f=f):
            assert prep is None and out is None
            return f(qkv.double(), nh, *arg).to(qkv.dtype)

        def vjp(qkv, g_out, nh, *arg, f=f, kind=kind):
            seen.append((kind, qkv, g_out))
            x = qkv.double().requires_grad_()
            with torch.enable_grad():
                g, = torch.autograd.grad(f(x, nh, *arg), x, g_out.double())
            return g.float()

        def jvp(qkv, qkv_dot, nh, *arg, f=f):
            assert qkv.dtype == qkv_dot.dtype == torch.float32 and qkv.is_contiguous() and qkv_dot.is_contiguous()
            o, od = torch.autograd.functional.jvp(lambda x: f(x, nh, *arg), qkv.double(), qkv_dot.double())
            return o.float(), od.float()

        monkeypatch.setattr(KD.ops, f"attn_{kind}", fwd)
        monkeypatch.setattr(KD.ops, f"attn_{kind}_vjp", vjp)
        monkeypatch.setattr(KD.ops, f"attn_{kind}_jvp", jvp)
    monkeypatch.setattr(KD.ops, "_prec_of", lambda x: KD._native.PREC_BF16 if x.dtype == torch.bfloat16 else KD._native.PREC_EXACT)
    monkeypatch.setattr(KD.compat, "_check", lambda q, what: None)
    return KD, seen


CASES = [("na2d", 7, 9, 11), ("flash", None, 7, 9), ("sdpa", None, 7, 9), ("window", (4, 2), 8, 12)]
# what the fakes hand back is the fp64 result rounded to fp32 (2^-24), at an operand whose q went through one fp32 multiply (a relative
# 2^-24 on logits of magnitude <= 10): a few 1e-7 in all
TOL = 1e-5


@pytest.mark.parametrize("scale", [1.0, None, 0.3])
@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_gradients_in_every_layout(fake, name, arg, H, W, scale):
    KD, seen = fake
    r = reference(name, arg, H, W, scale, 5, torch.float32)
    ins = r.op.views(r.proj.clone().requires_grad_())
    out = r.op.call(KD.compat, ins, scale)
    assert out.shape == r.out.shape and out.dtype == torch.float32 and relerr64(out, r.out) < TOL
    with torch.no_grad():
        assert torch.equal(out, r.op.call(KD.compat, ins, scale))
    grads = torch.autograd.grad(out, ins, r.g_out)
    for got, want in zip(grads, r.grads):
        assert got.shape == want.shape and got.dtype == torch.float32
    for part, (got, want) in enumerate(zip(slots(grads), slots(r.grads))):
        assert relerr64(got, want) < TOL, (part, relerr64(got, want))
    # what reached the kernel: one contiguous fp32 [.., 3 * nh * 64] operand, q already times the scale, and the gradient as [.., nh * 64]
    (kind, qkv, g_out), = seen
    assert kind == {"na2d": "na2d", "window": "window"}.get(name, "global")
    assert qkv.dtype == g_out.dtype == torch.float32 and qkv.is_contiguous() and g_out.is_contiguous()
    lead = (N, H, W) if kind != "global" else (N, H * W)
    assert qkv.shape == (*lead, 3 * NH * E) and g_out.shape == (*lead, NH * E)
    q, k, v = (t.detach().reshape(*lead, NH * E) for t in heads_last(name, slots(ins)))
    eff = DEFAULT_SCALE if scale is None else scale
    assert torch.equal(qkv, torch.cat([q * eff if eff != 1.0 else q, k, v], dim=-1))


def heads_last(name, qkv):
    """q, k, v of an operator's layout as [.., nh, 64]."""
    if name == "sdpa":
        return tuple(t.transpose(1, 2) for t in qkv)
    if name == "window":
        return tuple(t.permute(0, 2, 3, 1, 4) for t in qkv)
    return tuple(qkv)


@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_saved_tensor_is_the_packed_operand_alone(fake, name, arg, H, W):
    KD, _ = fake
    for dtype in (torch.float32, torch.bfloat16):
        ins = operator(name, arg, H, W).views(projection(H, W, 6).to(dtype).requires_grad_())
        out = operator(name, arg, H, W).call(KD.compat, ins, 0.3)
        assert out.dtype == dtype
        saved = attention_node(out).saved_tensors
        assert len(saved) == 1 and saved[0].dtype == dtype and saved[0].shape[-1] == 3 * NH * E and saved[0].is_contiguous()
        assert saved[0].untyped_storage().data_ptr() != ins[0].untyped_storage().data_ptr()      # not the caller's memory
        grads = torch.autograd.grad(out, ins, torch.ones_like(out))
        assert all(g.dtype == dtype for g in grads)


@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_no_graph_without_a_derivative(fake, name, arg, H, W):
    KD, seen = fake
    op = operator(name, arg, H, W)
    out = op.call(KD.compat, op.views(projection(H, W, 6)), 1.0)
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        out = op.call(KD.compat, op.views(projection(H, W, 6).requires_grad_()), 1.0)
    assert out.grad_fn is None and not out.requires_grad and not seen


@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_partial_gradients_and_inplace_safety(fake, name, arg, H, W):
    KD, seen = fake
    r = reference(name, arg, H, W, 0.3, 5, torch.float32)
    if name != "flash":
        for part in (2, 0):                                 # only v requires grad, then only q
            ins = tuple(t.detach().requires_grad_(i == part) for i, t in enumerate(r.op.views(r.proj.clone())))
            assert not ins[part].is_contiguous()
            out = r.op.call(KD.compat, ins, 0.3)
            handed = attention_node(out).apply(heads_last(name, (r.g_out,))[0].contiguous())
            assert [g is not None for g in handed] == [i == part for i in range(6)]        # nothing for the others
            got, = torch.autograd.grad(out, ins[part], r.g_out)
            assert relerr64(got, r.grads[part]) < TOL
        assert len(seen) == 4                               # one launch per backward
    # q and k modified in place after the call (the reference rotates them in place around it): backward is unaffected
    leaf = r.proj.clone().requires_grad_()
    ins = r.op.views(leaf * 1.0)
    out = r.op.call(KD.compat, ins, 0.3)
    with torch.no_grad():
        for t in slots(ins)[:2]:
            t.mul_(-2.0)
    got, = torch.autograd.grad(out, leaf, r.g_out)
    want = torch.cat([t.reshape(N, H, W, NH * E) for t in heads_last(name, slots(r.grads))], dim=-1)
    assert relerr64(got, want) < TOL


@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_double_backward_raises(fake, name, arg, H, W):
    KD, _ = fake
    op = operator(name, arg, H, W)
    ins = op.views(projection(H, W, 6).requires_grad_())
    out = op.call(KD.compat, ins, 1.0)
    grads = torch.autograd.grad(out, ins, torch.ones_like(out), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(grads[0].sum(), ins)


@pytest.mark.parametrize("scale", [1.0, None, 0.3])
@pytest.mark.parametrize("name,arg,H,W", CASES)
def test_tangents_in_every_layout(fake, name, arg, H, W, scale):
    KD, _ = fake
    r = reference(name, arg, H, W, scale, 5, torch.float32)
    want, want_v = reference_jvp(name, arg, H, W, scale, 5, torch.float32)
    plain = r.op.call(KD.compat, r.op.views(r.proj), scale)
    with forward_ad.dual_level():
        out = r.op.call(KD.compat, tuple(forward_ad.make_dual(p, t) for p, t in zip(r.op.views(r.proj), r.tangents)), scale)
        primal, o_dot = forward_ad.unpack_dual(out)
        assert torch.equal(primal, plain) and o_dot.shape == want.shape and relerr64(o_dot, want) < TOL, relerr64(o_dot, want)
        ins = r.op.views(r.proj)
        if name == "flash":
            duals = (forward_ad.make_dual(ins[0], v_only(r.tangents)[0]),)
        else:
            duals = (ins[0], ins[1], forward_ad.make_dual(ins[2], r.tangents[2]))           # q and k carry no tangent at all
        o_dot = forward_ad.unpack_dual(r.op.call(KD.compat, duals, scale)).tangent
        assert relerr64(o_dot, want_v) < TOL, relerr64(o_dot, want_v)


def test_import_shims():
    from k_diffusion_amd import compat
    from k_diffusion_amd.compat import flash_attn, natten                 # the statement INTEGRATION.md gives
    assert natten.has_fused_na() is True and callable(natten.functional.na2d) and callable(flash_attn.flash_attn_qkvpacked_func)
    natten, flash_attn = compat.natten, compat.flash_attn
    assert natten.has_fused_na() is True
    assert natten.functional.na2d is compat.na2d and flash_attn.flash_attn_qkvpacked_func is compat.flash_attn_qkvpacked_func
    assert compat.D_HEAD == 64 and callable(compat._split_stored)


def test_window_refusals_name_their_argument(fake):
    KD, _ = fake
    q = torch.zeros(1, 1, 8, 12, 64)
    with pytest.raises(NotImplementedError, match="window_size"):
        KD.compat.apply_window_attention(6, 0, q, q, q)
    with pytest.raises(NotImplementedError, match="window_shift"):
        KD.compat.apply_window_attention(4, 1, q, q, q)
    q = torch.zeros(1, 1, 10, 12, 64)
    with pytest.raises(NotImplementedError, match=r"\bH\b"):
        KD.compat.apply_window_attention(4, 0, q, q, q)

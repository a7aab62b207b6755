"""Derivatives of the k_diffusion_amd.compat operators on the MI355X: gradients (``torch.autograd``) and tangents (``forward_ad``) of
na2d, flash_attn_qkvpacked_func, scaled_dot_product_attention and apply_window_attention, each in the reference's own layout on the
strided views the reference's blocks produce, against the CPU oracle under autograd in fp64.

Tolerances (tests/helpers.relerr: max-abs over max-abs, per q / k / v slot).  fp32 tensors: 1e-5, the bound tests/test_vjp_gpu.py holds
these same kernels to on this same input recipe (the wrappers add a concatenation, slices and at most one fp32 multiply).  bf16 tensors:
2^-8 against the fp64 derivative at the bf16-rounded inputs -- the derivative kernels run in fp32 on the widened operand, so the only
rounding beyond the fp32 case is the final cast to bf16, whose unit roundoff 2^-8 is relative to each element and so at most that of the
largest.  Shapes: the smallest at which the kernels change path (every kernel-size
class of the neighbourhood kernels, T <= 256 and the streamed form above it, both window sizes with and without the shift)."""
import pytest
import torch
from torch.autograd import forward_ad

from oracle import hdit
from tests.helpers import relerr
from tests.test_compat_grad_cpu import E, N, NH, attention_node, heads_last, reference, reference_jvp, slots, v_only

pytestmark = pytest.mark.gpu
DEV = "cuda"
KTOL = 1e-5
BTOL = 2.0 ** -8
SEED = 11

NA2D = [("na2d", ks, H, W) for ks, H, W in ((3, 9, 11), (7, 9, 11), (13, 13, 17))]
GLOBAL = [(name, None, H, W) for name in ("flash", "sdpa") for H, W in ((7, 9), (12, 25))]              # T = 63, and 300 > 256: streamed
WINDOW = [("window", (ws, shift), H, W) for ws, H, W in ((4, 8, 12), (8, 16, 8)) for shift in (0, ws // 2)]
CASES = [(*c, s) for c in NA2D for s in (1.0, None, 0.3)] + [(*c, s) for c in GLOBAL + WINDOW for s in (1.0, None)]
ONE_EACH = [("na2d", 7, 9, 11, 0.3), ("flash", None, 7, 9, None), ("sdpa", None, 12, 25, 1.0), ("window", (4, 2), 8, 12, None)]


def ids(case):
    return "-".join(str(c).replace(" ", "") for c in case)


@pytest.fixture(params=["fp32-split3", "fp32-exact", "bf16"])
def mode(request, monkeypatch):
    """Tensor dtype and, for fp32 tensors, the arithmetic mode of the forward core -> (dtype, tolerance, exact)."""
    monkeypatch.setenv("KDIFF_GEMM", "exact" if request.param == "fp32-exact" else "split3")
    if request.param == "bf16":
        return torch.bfloat16, BTOL, False
    return torch.float32, KTOL, request.param == "fp32-exact"


def refused_in_exact_mode(KD, r, name, arg, H, W, exact):
    """The limits of the exact-fp32 forward cores, which the derivative route keeps as they are: the neighbourhood core takes kernel size
    7 only (compat's NotImplementedError), the dense core at most 256 tokens (the library's error; above it only the streamed split3 core)."""
    if exact and name == "na2d" and arg != 7:
        error, text = NotImplementedError, "kernel_size 7"
    elif exact and name in ("flash", "sdpa") and H * W > 256:
        error, text = RuntimeError, "256 tokens"
    else:
        return False
    with pytest.raises(error, match=text):
        r.op.call(KD.compat, r.op.views(r.proj.to(DEV).requires_grad_()), r.scale)
    return True


@pytest.mark.parametrize("name,arg,H,W,scale", CASES, ids=map(ids, CASES))
def test_reverse_mode(KD, mode, name, arg, H, W, scale):
    """Gradients in the operator's own layout against fp64; the output under grad is the output under no_grad, bit for bit, and comes
    from one _Attention node that holds the packed operand alone; backward is deterministic."""
    dtype, tol, exact = mode
    r = reference(name, arg, H, W, scale, SEED, dtype)
    if refused_in_exact_mode(KD, r, name, arg, H, W, exact):
        return
    ins = r.op.views(r.proj.to(DEV).requires_grad_())
    assert not ins[-1].is_contiguous() or name == "flash"
    out = r.op.call(KD.compat, ins, scale)
    assert out.shape == r.out.shape and out.dtype == dtype and out.requires_grad
    with torch.no_grad():
        plain = r.op.call(KD.compat, ins, scale)
    assert plain.grad_fn is None and torch.equal(out, plain)
    saved = attention_node(out).saved_tensors
    assert len(saved) == 1 and saved[0].dtype == dtype and saved[0].shape[-1] == 3 * NH * E
    grads = torch.autograd.grad(out, ins, r.g_out.to(DEV), retain_graph=True)
    for part, (got, want) in enumerate(zip(slots(grads), slots(r.grads))):
        err = relerr(got, want)
        print(f"{name} {arg} {H}x{W} scale {scale} {dtype}: slot {part} relerr {err:.3e}")
        assert got.shape == want.shape and got.dtype == dtype and err < tol, (part, err)
    again = torch.autograd.grad(out, ins, r.g_out.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(grads, again))


@pytest.mark.parametrize("name,arg,H,W,scale", ONE_EACH, ids=map(ids, ONE_EACH))
def test_partial_inplace_and_double_backward(KD, mode, name, arg, H, W, scale):
    dtype, _, exact = mode
    r = reference(name, arg, H, W, scale, SEED, dtype)
    if refused_in_exact_mode(KD, r, name, arg, H, W, exact):
        return
    g_out = r.g_out.to(DEV)
    leaf = r.proj.to(DEV).requires_grad_()
    ins = r.op.views(leaf)
    full = torch.autograd.grad(r.op.call(KD.compat, ins, scale), ins, g_out)
    # only v requires grad, then only q: the same values, and the node hands nothing back for the others
    if name != "flash":
        for part in (2, 0):
            some = tuple(t.detach().requires_grad_(i == part) for i, t in enumerate(r.op.views(r.proj.to(DEV))))
            out = r.op.call(KD.compat, some, scale)
            handed = attention_node(out).apply(heads_last(name, (g_out,))[0].contiguous())
            assert [g is not None for g in handed] == [i == part for i in range(6)]
            got, = torch.autograd.grad(out, some[part], g_out)
            assert torch.equal(got, full[part])
    # q and k modified in place after the call, as the reference's apply_rotary_emb_ does around it: the same gradient
    want, = torch.autograd.grad(r.op.call(KD.compat, r.op.views(leaf * 1.0), scale), leaf, g_out)
    ins = r.op.views(leaf * 1.0)
    out = r.op.call(KD.compat, ins, scale)
    with torch.no_grad():
        for t in slots(ins)[:2]:
            t.mul_(-2.0)
    got, = torch.autograd.grad(out, leaf, g_out)
    assert torch.equal(got, want)
    assert torch.equal(got, torch.cat([t.reshape(N, H, W, NH * E) for t in heads_last(name, slots(full))], dim=-1))
    # first derivatives only
    ins = r.op.views(r.proj.to(DEV).requires_grad_())
    grads = torch.autograd.grad(r.op.call(KD.compat, ins, scale), ins, g_out, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(grads[0].sum(), ins)


@pytest.mark.parametrize("name,arg,H,W,scale", CASES, ids=map(ids, CASES))
def test_forward_mode(KD, mode, name, arg, H, W, scale):
    """Tangents on q, k and v, and on v alone, against fp64 torch.autograd.functional.jvp of the oracle; the primal is the plain forward."""
    dtype, tol, exact = mode
    r = reference(name, arg, H, W, scale, SEED, dtype)
    if refused_in_exact_mode(KD, r, name, arg, H, W, exact):
        return
    want, want_v = reference_jvp(name, arg, H, W, scale, SEED, dtype)
    ins = r.op.views(r.proj.to(DEV))
    plain = r.op.call(KD.compat, ins, scale)
    assert plain.grad_fn is None
    tangents = r.op.views(torch.cat([t.reshape(N, H, W, NH * E) for t in heads_last(name, slots(r.tangents))], dim=-1).to(DEV))    # strided too
    with forward_ad.dual_level():
        out = r.op.call(KD.compat, tuple(forward_ad.make_dual(p, t) for p, t in zip(ins, tangents)), scale)
        primal, o_dot = forward_ad.unpack_dual(out)
        err = relerr(o_dot, want)
        print(f"{name} {arg} {H}x{W} scale {scale} {dtype}: o_dot relerr {err:.3e}")
        assert torch.equal(primal, plain) and o_dot.shape == want.shape and o_dot.dtype == dtype and err < tol, err
        if name == "flash":
            duals = (forward_ad.make_dual(ins[0], v_only(r.tangents)[0].to(DEV)),)
        else:
            duals = (ins[0], ins[1], forward_ad.make_dual(ins[2], tangents[2]))            # q and k carry no tangent at all
        primal, o_dot = forward_ad.unpack_dual(r.op.call(KD.compat, duals, scale))
        err = relerr(o_dot, want_v)
        print(f"{name} {arg} {H}x{W} scale {scale} {dtype}: o_dot (v only) relerr {err:.3e}")
        assert torch.equal(primal, plain) and err < tol, err


@pytest.mark.parametrize("name,arg,H,W,scale", ONE_EACH, ids=map(ids, ONE_EACH))
def test_adjoint_identity(KD, monkeypatch, name, arg, H, W, scale):
    """<g, J t> from forward mode against <J^T g, t> from reverse mode, fp32 tensors; 1e-4 is the bound tests/test_vjp_gpu.py holds the
    model-level input gradient to in exact mode -- looser than these kernels need, it documents intent."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    r = reference(name, arg, H, W, scale, SEED, torch.float32)
    ins = r.op.views(r.proj.to(DEV).requires_grad_())
    g, tangents = r.g_out.to(DEV), tuple(t.to(DEV) for t in r.tangents)
    grads = torch.autograd.grad(r.op.call(KD.compat, ins, scale), ins, g)
    with forward_ad.dual_level():
        duals = tuple(forward_ad.make_dual(p.detach(), t) for p, t in zip(ins, tangents))
        o_dot = forward_ad.unpack_dual(r.op.call(KD.compat, duals, scale)).tangent
    lhs = (g.double() * o_dot.double()).sum().item()
    rhs = sum((a.double() * t.double()).sum().item() for a, t in zip(grads, tangents))
    gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"{name}: <g, J t> = {lhs:.9e}, <J^T g, t> = {rhs:.9e}, relative gap {gap:.3e}")
    assert gap < 1e-4, gap


# ---- one attention block end to end -----------------------------------------------------------------------------------------------------------

def _block(x, w_qkv, head_scale, w_out, attention, H, W):
    """x [n, h, w, d] -> bias-free qkv projection -> heads -> cosine-sim scaled q, k -> attention -> bias-free out projection -> sum of
    squares; ``attention`` maps q, k, v [n, h, w, nh, e] to [n, h, w, nh, e]."""
    q, k, v = (x @ w_qkv.T).view(N, H, W, 3, NH, E).unbind(3)
    q, k = hdit.cosine_sim_scale(q, k, head_scale)
    y = attention(q, k, v).reshape(N, H, W, NH * E) @ w_out.T
    return y.square().sum()


def _block_inputs(H, W):
    gen = torch.Generator().manual_seed(23)
    d = NH * E
    x = torch.randn(N, H, W, d, generator=gen)
    w_qkv, w_out = torch.randn(3 * d, d, generator=gen) * d ** -0.5, torch.randn(d, d, generator=gen) * d ** -0.5
    return x, w_qkv, torch.linspace(6.0, 12.0, NH), w_out


def _block_grads(params, attention, H, W, device, dtype):
    params = tuple(p.to(device, dtype).requires_grad_() for p in params)
    return torch.autograd.grad(_block(*params, attention, H, W), params)


def test_block_with_the_natten_shim(KD, monkeypatch):
    """Gradients of both weights, the per-head scale and x through a neighbourhood block on the device (compat.natten in fp32, the rest
    torch) against the same block on the CPU in fp64 with the oracle's na2d."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    natten = KD.compat.natten
    assert natten.has_fused_na() is True
    H, W = 9, 11
    params = _block_inputs(H, W)
    want = _block_grads(params, lambda q, k, v: hdit.na2d(q, k, v, 7, 1.0), H, W, "cpu", torch.float64)
    got = _block_grads(params, lambda q, k, v: natten.functional.na2d(q, k, v, 7, scale=1.0), H, W, DEV, torch.float32)
    for what, a, b in zip(("x", "w_qkv", "head scale", "w_out"), got, want):
        print(f"na2d block: d loss / d {what} relerr {relerr(a, b):.3e}")
        assert relerr(a, b) < 1e-4, (what, relerr(a, b))


def test_block_with_the_flash_attn_shim(KD, monkeypatch):
    """The same block with compat.flash_attn in bf16 (the reference runs flash-attn under bf16 autocast: qkv is rounded to bf16 in front
    of it, the rest stays fp32), against the fp64 block fed the same bf16-rounded qkv.

    Bound: the loss gradient that enters the attention backward is 2 y W_out and so carries the error of the bf16 forward core, which the
    project holds to 2e-2 against the oracle (tests/test_ops_gpu.py, the compat forward test in bf16); the backward itself adds the one
    rounding of its result to bf16, 2^-8 per operator as above.  Everything after is linear in those two, so 2e-2 + 2^-8."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    flash_attn = KD.compat.flash_attn
    H, W = 7, 9
    params = _block_inputs(H, W)
    rounded = []

    def on_device(q, k, v):
        qkv = torch.stack([t.reshape(N, H * W, NH, E) for t in (q, k, v)], dim=2).to(torch.bfloat16)
        rounded.append(qkv.detach())
        return flash_attn.flash_attn_qkvpacked_func(qkv, softmax_scale=1.0).float().view(N, H, W, NH, E)

    def on_cpu(q, k, v):
        qkv = torch.stack([t.reshape(N, H * W, NH, E) for t in (q, k, v)], dim=2)
        qkv = qkv + (rounded[0].cpu().double() - qkv).detach()            # the device's bf16 values; the rounding's derivative is one
        return hdit.attn_global(*(t.reshape(N, H, W, NH, E) for t in qkv.unbind(2)), 1.0)

    got = _block_grads(params, on_device, H, W, DEV, torch.float32)
    want = _block_grads(params, on_cpu, H, W, "cpu", torch.float64)
    for what, a, b in zip(("x", "w_qkv", "head scale", "w_out"), got, want):
        print(f"flash block: d loss / d {what} relerr {relerr(a, b):.3e}")
        assert relerr(a, b) < 2e-2 + BTOL, (what, relerr(a, b))


def test_window_refusals_name_their_argument(KD):
    q = torch.zeros(1, 1, 8, 12, 64, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="window_size"):
        KD.compat.apply_window_attention(6, 0, q, q, q)
    with pytest.raises(NotImplementedError, match="window_shift"):
        KD.compat.apply_window_attention(4, 1, q, q, q)
    q = torch.zeros(1, 1, 10, 12, 64, device=DEV)
    with pytest.raises(NotImplementedError, match=r"\bH\b"):
        KD.compat.apply_window_attention(4, 0, q, q, q)
    with pytest.raises(NotImplementedError):                      # the masked SDPA call stays refused: the window operator replaces it
        KD.compat.scaled_dot_product_attention(*(torch.zeros(1, 1, 16, 64, device=DEV),) * 3, attn_mask=torch.ones(16, 16, dtype=torch.bool, device=DEV))

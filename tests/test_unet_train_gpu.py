"""Training the image_v1 U-Net on the MI355X: the convolution's weight-gradient kernel (csrc/conv_wgrad_x3.hip), the small parameter-gradient
rules (csrc/unet_train_f32.hip), ``Denoiser.loss`` with ``backward()`` through ``ImageDenoiserModelV1.loss_forward``, one optimizer step, and the
refusals.  Truth is fp64 on the CPU: ``torch.nn.grad.conv2d_weight``, autograd of ``adagn_expr`` / ``F.gelu``, and autograd over the restated loss
(tests/unet_train_ref.py), which tests/test_unet_train_cpu.py ties to the REAL reference's recorded numbers.

Bounds.
* conv weight gradient: the project's split3 weight-gradient bound (tests/test_param_grad_gpu.py), 2e-5 of the largest entry.
* AdaGN (w, b) gradient, GELU reverse, bias gradient: 1e-5 of the largest entry, the project's bound for its fp64-sum reductions.
* model: losses within 1e-5 relative of fp64 autograd; every parameter gradient within 5e-4 (max-abs relative per tensor), the family's gate.
"""
import functools

import pytest
import torch
from torch.nn import functional as F

from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.test_unet_gpu import DEV, adagn_expr, built, g, rel, rn, tokens
from tests.test_unet_train_cpu import restated

pytestmark = pytest.mark.gpu
WGRAD_BOUND = 2e-5
SUM_BOUND = 1e-5
TRAIN_KERNELS = ("conv2d_wgrad", "adagn_wb_grad", "gelu_vjp", "bias_grad", "wgrad_", "colsum")


def prof_names(nat):
    import ctypes as C
    lib, out = nat.lib(), []
    name, ms, fl, by = C.create_string_buffer(128), C.c_float(), C.c_double(), C.c_double()
    for i in range(lib.kd_prof_count()):
        nat.check(lib.kd_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)), "kd_prof_get")
        out.append(name.value.decode())
    return out


def profiled(nat, fn):
    """(fn(), the names of the launches it made)"""
    lib = nat.lib()
    lib.kd_prof_reset()
    lib.kd_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = prof_names(nat)
    finally:
        lib.kd_prof_enable(0)
        lib.kd_prof_reset()
    return out, names


# ---- 1. the convolution's weight gradient ----------------------------------------------------------------------------------------------------

# (B, (H, W), c_in, c_out, ks, layout): "a_lo" / "a_hi" = A is the left / right 128-column half of a 256-wide buffer; "g_hi" = G is the right half
WGRAD_CASES = [(2, (12, 20), 64, 128, 3, "plain"),         # ragged patches on both axes
               (2, (12, 20), 64, 128, 3, "g_hi"),          # ... with G a column range (the gradient of a level's skip)
               (3, (7, 7), 128, 64, 3, "plain"),           # an image smaller than a patch
               (1, (2, 2), 64, 64, 3, "plain"),            # the smallest legal level, mostly padding: one patch, one chunk
               (2, (16, 8), 128, 192, 1, "a_lo"),          # ks = 1 with row strides
               (2, (16, 8), 128, 192, 1, "a_hi"),
               (5, (56, 8), 256, 256, 3, "plain")]         # 35 patches in 12 chunks of 3, the last one of 2 (conv_wgrad_chunks)


@functools.lru_cache(maxsize=None)
def wgrad_reference(B, hw, ci, co, ks):
    """(a, g, dW in fp64): computed once per shape."""
    H, W = hw
    a, gy = rn(B, ci, H, W, seed=ci + 7 * H + W), rn(B, co, H, W, seed=co + 11 * H + W + 1)
    ref = torch.nn.grad.conv2d_weight(a.double(), (co, ci, ks, ks), gy.double(), padding=ks // 2)
    return a, gy, ref


def _operand(t, layout, which):
    """The device operand of tokens t under a layout: plain, or one half of a NaN-filled buffer of twice the width."""
    t = g(t)
    side = {"a_lo": ("a", 0), "a_hi": ("a", 1), "g_hi": ("g", 1)}.get(layout)
    if side is None or side[0] != which:
        return t
    C = t.shape[1]
    buf = torch.full((t.shape[0], 2 * C), float("nan"), device=DEV)
    buf[:, side[1] * C:(side[1] + 1) * C] = t
    return buf[:, side[1] * C:(side[1] + 1) * C]


@pytest.mark.parametrize("B,hw,ci,co,ks,layout", WGRAD_CASES, ids=str)
def test_conv_wgrad_matches_fp64(KD, B, hw, ci, co, ks, layout):
    uo = KD.unet_ops
    a, gy, ref = wgrad_reference(B, hw, ci, co, ks)
    at, gt = _operand(tokens(a), layout, "a"), _operand(tokens(gy), layout, "g")
    per, n = uo.conv_wgrad_chunks(B, *hw, ci, co)
    patches = B * -(-hw[0] // 8) * -(-hw[1] // 8)
    (dw, names) = profiled(KD._native, lambda: uo.conv2d_wgrad(gt, at, B, *hw, ks))
    err = (dw.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"conv wgrad B{B} {hw[0]}x{hw[1]} {ci}->{co} k{ks} {layout}: {err:.3e} of the largest ({WGRAD_BOUND:.0e}); {n} chunk(s) of {per} patches; {names}")
    assert dw.shape == (co, ci, ks, ks) and err < WGRAD_BOUND
    assert any(nm.startswith(f"conv2d_wgrad_x3<k{ks}>") and nm.endswith(f"chunks={n}") for nm in names), names
    if B == 5:
        assert n >= 3 and patches % per, "not the multi-chunk shape with a ragged last chunk"
    if hw == (2, 2):
        assert n == 1
    assert torch.equal(uo.conv2d_wgrad(gt, at, B, *hw, ks), dw), "a repeat gives other bits"
    # accumulate: added to what out holds -- dW is far from a multiple of the rounding of out + dW, so bits cannot be asked for
    acc0 = g(rn(co, ci, ks, ks, seed=5))
    acc = uo.conv2d_wgrad(gt, at, B, *hw, ks, out=acc0.clone(), accumulate=True)
    e_acc = (acc.cpu().double() - (ref + acc0.cpu().double())).abs().max().item() / ref.abs().max().item()
    assert e_acc < WGRAD_BOUND, e_acc
    # another cut of the sum, the same gradient: two chunks (or one), within the bound of the first
    other = uo.conv2d_wgrad(gt, at, B, *hw, ks, chunks=(-(-patches // 2), 2 if patches > 1 else 1))
    assert (other.cpu().double() - ref).abs().max().item() / ref.abs().max().item() < WGRAD_BOUND
    # the folded 1 / 8 of a qkv projection's q rows: exact
    q = uo.conv2d_wgrad(gt, at, B, *hw, ks, q_rows=64)
    assert torch.equal(q[:64], dw[:64] * 0.125) and torch.equal(q[64:], dw[64:])


@pytest.mark.parametrize("ks", [3, 1])
def test_conv_wgrad_one_hot_lights_one_tap(KD, ks):
    """A one-hot pixel / channel in A and in G lights exactly one (co, ci, ky, kx): a flipped or transposed tap shows."""
    uo = KD.unet_ops
    B, H, W, ci, co = 2, 9, 11, 128, 64
    taps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if ks == 3 else [(0, 0)]
    for n, (dy, dx) in enumerate(taps):
        b, y, x, c_a, c_g = n % B, 8 if dy < 0 else 7, 8 + (n % 2), (37 + 5 * n) % ci, (11 + 3 * n) % co      # across the patch boundary at 8
        a, gy = torch.zeros(B, H, W, ci), torch.zeros(B, H, W, co)
        gy[b, y, x, c_g] = 2.0
        a[b, y + dy, x + dx, c_a] = 0.75                                 # G[y, x] meets A[y + ky - h, x + kx - h]: ky = dy + h
        dw = uo.conv2d_wgrad(g(gy.reshape(-1, co)), g(a.reshape(-1, ci)), B, H, W, ks).cpu()
        want = torch.zeros(co, ci, ks, ks)
        want[c_g, c_a, dy + ks // 2, dx + ks // 2] = 1.5
        assert torch.equal(dw, want), f"tap ({dy}, {dx}): lit {dw.nonzero().tolist()}, expected {want.nonzero().tolist()}"
    # the same pixel in another sample does not meet it
    a, gy = torch.zeros(B, H, W, ci), torch.zeros(B, H, W, co)
    gy[0, 4, 4, 1], a[1, 4, 4, 2] = 1.0, 1.0
    assert not bool(uo.conv2d_wgrad(g(gy.reshape(-1, co)), g(a.reshape(-1, ci)), B, H, W, ks).any())


def test_conv_wgrad_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    gt, at = g(rn(2 * 16, 64)), g(rn(2 * 16, 64, seed=1))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        uo.conv2d_wgrad(g(rn(32, 96)), at, 2, 4, 4, 3)
    with pytest.raises(RuntimeError, match="kernel size"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 5)
    with pytest.raises(RuntimeError, match="do not cut"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 3, chunks=(1, 3))
    with pytest.raises(ValueError, match="rows for batch"):
        uo.conv2d_wgrad(gt, at, 2, 4, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.conv2d_wgrad(gt.cpu(), at, 2, 4, 4, 3)
    with pytest.raises(ValueError, match="accumulate needs"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 3, accumulate=True)


# ---- 2. the small rules --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "plain"])
def test_adagn_wb_grad_matches_fp64(KD, gelu):
    uo = KD.unet_ops
    B, H, W, chan, groups = 2, 6, 10, 128, 4
    x, w, b, gy = 1.5 * rn(B, chan, H, W, seed=3) + 0.3, 0.5 * rn(B, chan, seed=4), 0.5 * rn(B, chan, seed=5), rn(B, chan, H, W, seed=6)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    gw64, gb64 = torch.autograd.grad(adagn_expr(x.double(), w64, b64, groups, gelu), (w64, b64), gy.double())
    ref = torch.cat([gw64, gb64], dim=1)
    xt, gyt, wb = g(tokens(x)), g(tokens(gy)), g(torch.cat([w, b], dim=1))
    stats = uo.groupnorm_stats(xt, B, groups)
    table = torch.full((B, 2 * chan + 192), -7.0, device=DEV)           # the norm's column range of a wider gradient table
    out = uo.adagn_wb_grad(xt, stats, wb, gyt, gelu=gelu, out=table[:, 64:64 + 2 * chan])
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"adagn (w, b) gradient gelu={gelu}: {err:.3e} of the largest ({SUM_BOUND:.0e})")
    assert err < SUM_BOUND
    assert bool((table[:, :64] == -7.0).all()) and bool((table[:, 64 + 2 * chan:] == -7.0).all()), "the columns beside the range were written"
    assert torch.equal(uo.adagn_wb_grad(xt, stats, wb, gyt, gelu=gelu), out), "a repeat gives other bits"
    # operands that are column ranges themselves
    wide = torch.full((xt.shape[0], 2 * chan), float("nan"), device=DEV)
    wide[:, chan:] = xt
    assert torch.equal(uo.adagn_wb_grad(wide[:, chan:], stats, wb, gyt, gelu=gelu), out)


def test_gelu_vjp_matches_fp64(KD):
    uo = KD.unet_ops
    pre, gy = 3.0 * rn(3, 70, seed=1), rn(3, 70, seed=2)
    p64 = pre.double().requires_grad_(True)
    ref = torch.autograd.grad(F.gelu(p64), p64, gy.double())[0]
    out = uo.gelu_vjp(g(pre), g(gy))
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"gelu reverse: {err:.3e} of the largest ({SUM_BOUND:.0e})")
    assert err < SUM_BOUND
    inplace = g(gy)
    assert uo.gelu_vjp(g(pre), inplace, out=inplace) is inplace and torch.equal(inplace, out)


@pytest.mark.parametrize("layout", ["tokens", "strided", "nchw"])
def test_bias_grad_matches_fp64(KD, layout):
    uo = KD.unet_ops
    B, H, W, chan = 3, 13, 17, 3 if layout == "nchw" else 192          # 663 rows: three runs of 256, the last ragged
    gy = rn(B, chan, H, W, seed=9) + 0.25
    ref = gy.double().sum(dim=(0, 2, 3))
    if layout == "nchw":
        gt = g(gy)
    elif layout == "strided":
        buf = torch.full((B * H * W, 2 * chan), float("nan"), device=DEV)
        buf[:, chan:] = g(tokens(gy))
        gt = buf[:, chan:]
    else:
        gt = g(tokens(gy))
    out = uo.bias_grad(gt)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"bias gradient {layout}: {err:.3e} of the largest ({SUM_BOUND:.0e})")
    assert out.shape == (chan,) and err < SUM_BOUND
    assert torch.equal(uo.bias_grad(gt), out), "a repeat gives other bits"
    q = 1 if layout == "nchw" else 64
    folded = uo.bias_grad(gt, q_cols=q)
    assert torch.equal(folded[:q], out[:q] * 0.125) and torch.equal(folded[q:], out[q:])
    acc0 = g(rn(chan, seed=2))
    acc = uo.bias_grad(gt, out=acc0.clone(), accumulate=True)
    assert (acc.cpu().double() - (ref + acc0.cpu().double())).abs().max().item() / ref.abs().max().item() < SUM_BOUND


# ---- 3. the model: Denoiser.loss and backward() ---------------------------------------------------------------------------------------------------

def trainable(KD, name):
    """A fresh model with the synth weights whose parameters require grad, in eval mode (the tiny configs have dropout_rate 0 anyway)."""
    cfg, _, sd = built(name)
    model = KD.config.make_model(cfg).eval()
    model.load_state_dict(sd)
    return model.to(DEV)


def hip_loss(KD, model, name, weighting):
    x, noise, sigma, aug = tr.batch(name)
    kw = {} if aug is None else {"aug_cond": g(aug)}
    return KD.Denoiser(model, tr.SIGMA_DATA, weighting).loss(g(x), g(noise), g(sigma), **kw)


def grads_of(model):
    return {k: p.grad for k, p in model.named_parameters()}


def worst(grads, ref, scale=1.0):
    """(largest max-abs relative error per tensor, its name) of gradients against fp64 ones times ``scale``."""
    errs = {k: rel(grads[k], ref[k] * scale) for k in ref}
    k = max(errs, key=errs.get)
    return errs[k], k


@pytest.mark.parametrize("weighting", tr.WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_loss_and_parameter_gradients_match_fp64(KD, name, weighting, monkeypatch):
    model = trainable(KD, name)
    want_losses, want = restated(name, weighting)
    losses = hip_loss(KD, model, name, weighting)
    assert losses.shape == want_losses.shape and losses.requires_grad
    e_loss = ((losses.detach().cpu().double() - want_losses).abs() / want_losses.abs()).max().item()
    losses.mean().backward()
    grads = grads_of(model)
    assert sorted(grads) == sorted(want) and all(v is not None and v.shape == want[k].shape for k, v in grads.items())
    e_grad, k_grad = worst(grads, want)
    print(f"{name} {weighting}: losses {e_loss:.3e} (1e-5), worst gradient {e_grad:.3e} at {k_grad} (5e-4), {len(grads)} parameters")
    assert e_loss < 1e-5
    assert e_grad < 5e-4
    first = {k: v.clone() for k, v in grads.items()}
    # a second loss and backward accumulate into the existing .grad: exactly twice (a doubling is exact)
    hip_loss(KD, model, name, weighting).mean().backward()
    assert all(torch.equal(p.grad, 2 * first[k]) for k, p in model.named_parameters()), "a second backward did not accumulate the same bits"
    if weighting != "karras":
        return
    # .sum(): B times the mean's gradient
    model.zero_grad(set_to_none=True)
    hip_loss(KD, model, name, weighting).sum().backward()
    e_sum, k_sum = worst(grads_of(model), want, scale=float(want_losses.shape[0]))
    print(f"{name}: .sum() worst gradient {e_sum:.3e} at {k_sum}")
    assert e_sum < 5e-4
    # fp32-grade whatever KDIFF_GEMM says: the bf16 mode gives the same bits (as the forward's and forward_vjp's tests ask)
    monkeypatch.setenv("KDIFF_GEMM", "bf16")
    model.zero_grad(set_to_none=True)
    again = hip_loss(KD, model, name, weighting)
    again.mean().backward()
    assert torch.equal(again, losses) and all(torch.equal(p.grad, first[k]) for k, p in model.named_parameters())
    monkeypatch.delenv("KDIFF_GEMM")
    # a retained graph: the second backward recomputes the tape
    model.zero_grad(set_to_none=True)
    kept = hip_loss(KD, model, name, weighting).mean()
    kept.backward(retain_graph=True)
    kept.backward()
    assert all(torch.equal(p.grad, 2 * first[k]) for k, p in model.named_parameters())
    # without grad mode: the same losses, no graph
    with torch.no_grad():
        plain = hip_loss(KD, model, name, weighting)
    assert not plain.requires_grad and torch.equal(plain, losses)


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_callable_weighting(KD, name):
    weighting = lambda sigma: 1 / (1 + sigma)
    cfg, _, sd = built(name)
    model = trainable(KD, name)
    names = sorted(k for k, _ in model.named_parameters())
    leaves = tr.leaf_state(sd, set(names))
    x, noise, sigma, aug = tr.batch(name)
    want_losses = tr.losses(leaves, x, noise, sigma, aug, weighting)
    want = dict(zip(names, torch.autograd.grad(want_losses.mean(), [leaves[k] for k in names])))
    losses = hip_loss(KD, model, name, weighting)
    losses.mean().backward()
    e_loss = ((losses.detach().cpu().double() - want_losses.detach()).abs() / want_losses.detach().abs()).max().item()
    e_grad, k_grad = worst(grads_of(model), want)
    print(f"{name} callable weighting: losses {e_loss:.3e} (1e-5), worst gradient {e_grad:.3e} at {k_grad} (5e-4)")
    assert e_loss < 1e-5 and e_grad < 5e-4


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_frozen_parameters_cost_no_launches(KD, name):
    nat = KD._native
    model = trainable(KD, name)
    _, full_names = profiled(nat, lambda: hip_loss(KD, model, name, "karras").mean().backward())
    full = {k: v.clone() for k, v in grads_of(model).items()}
    model.zero_grad(set_to_none=True)
    frozen = [k for k, _ in model.named_parameters() if ".main.2." in k or "mapping" in k or "proj_in" in k or k.endswith("qkv_proj.bias")]
    assert frozen and len(frozen) < len(full)
    for k, p in model.named_parameters():
        p.requires_grad_(k not in frozen)
    _, part_names = profiled(nat, lambda: hip_loss(KD, model, name, "karras").mean().backward())
    for k, p in model.named_parameters():
        if k in frozen:
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, full[k]), f"{k}: other bits with a frozen subset"
    count = lambda names: sum(any(n.startswith(t) for t in TRAIN_KERNELS) for n in names)
    print(f"{name}: {len(full_names)} launches ({count(full_names)} for parameter gradients) with every parameter, {len(part_names)} "
          f"({count(part_names)}) with {len(frozen)} frozen")
    assert len(part_names) < len(full_names) and count(part_names) < count(full_names)
    # everything frozen: the plain primal, no gradient launch at all
    model.requires_grad_(False)
    out, none_names = profiled(nat, lambda: hip_loss(KD, model, name, "karras"))
    assert not out.requires_grad and count(none_names) == 0


def test_one_optimizer_step_then_sample(KD):
    """One K.optim.AdamW step on unet_b: the no-grad forward follows the updated weights (the plan and VJP caches dropped), and the loss on them
    matches fp64.  (Nothing is asserted about the loss falling: on this batch four reference AdamW steps raise it.)"""
    name = "unet_b"
    model = trainable(KD, name)
    x, noise, sigma, aug = tr.batch(name)
    xi, si, _ = ur.inputs(name)
    with torch.no_grad():
        before = model.requires_grad_(False)(g(xi), g(si)).clone()
        model.forward_vjp(g(xi), g(si))
    model.requires_grad_(True)
    opt = KD.optim.AdamW(model.param_groups(1e-3), lr=1e-3, betas=(0.95, 0.999), eps=1e-6, weight_decay=1e-3)
    old = {k: v.clone() for k, v in model.state_dict().items()}
    hip_loss(KD, model, name, "karras").mean().backward()
    opt.step(clip_grad_norm=1.0, zero_grad=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    moved = [k for k, _ in model.named_parameters() if not torch.equal(sd[k], old[k].cpu())]
    assert len(moved) == len(list(model.parameters())), "a parameter did not move"
    assert all(not bool(p.grad.any()) for p in model.parameters()), "zero_grad=True left a gradient"
    model.requires_grad_(False)
    with torch.no_grad():
        after = model(g(xi), g(si))
    ref = ur.forward(sd, xi, si)
    e_fwd = rel(after, ref)
    print(f"{name}: forward on the updated weights {e_fwd:.3e} from the restatement (5e-4); moved {rel(after, before.cpu()):.3e}")
    assert e_fwd < 5e-4 and not torch.equal(after, before)
    model.requires_grad_(True)
    want = tr.losses(tr.leaf_state(sd, set()), x, noise, sigma, aug, "karras")
    got = hip_loss(KD, model, name, "karras")
    e_loss = ((got.detach().cpu().double() - want).abs() / want.abs()).max().item()
    print(f"{name}: loss on the updated weights {e_loss:.3e} (1e-5)")
    assert e_loss < 1e-5
    # torch's own optimizer takes the same gradients
    got.mean().backward()
    torch.optim.AdamW(model.param_groups(2e-4)).step()


def test_refusals_on_the_device(KD):
    import json
    name = "unet_b"
    model = trainable(KD, name)
    x, noise, sigma, _ = tr.batch(name)
    den = KD.Denoiser(model, tr.SIGMA_DATA)
    for bad in ("input", "noise", "sigma"):
        args = {"input": g(x), "noise": g(noise), "sigma": g(sigma)}
        args[bad] = args[bad].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match=f"gradients w.r.t. {bad}"):
            den.loss(**args)
    wrapped = trainable(KD, "unet_a")
    xa, na, sa, aug = tr.batch("unet_a")
    with pytest.raises(NotImplementedError, match="gradients w.r.t. aug_cond"):
        KD.Denoiser(wrapped, tr.SIGMA_DATA).loss(g(xa), g(na), g(sa), aug_cond=g(aug).requires_grad_(True))
    with pytest.raises(NotImplementedError, match="mapping_cond gets no gradient"):
        wrapped.loss_forward(g(xa), g(sa), aug_cond=g(aug).requires_grad_(True))
    # the sampling passes keep their refusal with trainable parameters
    for call in (lambda: model(g(x), g(sigma)), lambda: model.forward_vjp(g(x), g(sigma)), lambda: model.forward_jvp(g(x), g(sigma), g(x)),
                 lambda: den(g(x), g(sigma))):
        with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
            call()
    raw = json.loads(json.dumps(ur.CONFIGS[name]))
    raw["model"]["dropout_rate"] = 0.05
    dropping = KD.config.make_model(KD.config.load_config(raw)).to(DEV)
    with pytest.raises(NotImplementedError, match=r"dropout_rate=0\.05.*model\.eval\(\)"):
        KD.Denoiser(dropping, tr.SIGMA_DATA).loss(g(x), g(noise), g(sigma))
    assert KD.Denoiser(dropping.eval(), tr.SIGMA_DATA).loss(g(x), g(noise), g(sigma)).requires_grad
    # the weights moved between the loss and its backward
    loss = den.loss(g(x), g(noise), g(sigma)).mean()
    with torch.no_grad():
        model.proj_in.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="weights changed between"):
        loss.backward()


# ---- 4. forward_vjp keeps its bits and its launch list -------------------------------------------------------------------------------------------

def test_forward_vjp_is_untouched_by_the_sink(KD):
    """The reverse walk that ``forward_vjp`` shares with the training backward: without a sink it launches none of the parameter-gradient kernels,
    and a sink that asks for every parameter leaves the activation gradients' bits alone -- the walk's launches are the same calls on the same
    operands, the sink's only read them.  (Against the parent commit itself: DESIGN.md section 8 records the digests.)"""
    import importlib
    name = "unet_b"
    _, model, _ = built(name)
    pkg = type(model).__module__.rsplit(".", 1)[0]                      # the copy of the package the model's classes come from
    unet_train, unet_vjp = importlib.import_module(pkg + ".unet_train"), importlib.import_module(pkg + ".unet_vjp")
    xi, si, _ = ur.inputs(name)
    u = g(rn(*xi.shape, seed=29))
    (out, grad), names = profiled(KD._native, lambda: (lambda o, pb: (o, pb(u)))(*model.forward_vjp(g(xi), g(si))))
    assert not any(n.startswith(t) for n in names for t in TRAIN_KERNELS), names
    with torch.no_grad():
        assert torch.equal(out, model(g(xi), g(si)))
        f, state = unet_train.primal(model, g(xi), g(si), None)
        assert torch.equal(f, out)
        sink = unet_train._Sink(model, state.c, list(model.parameters()))
        gt = KD.unet_ops.unet_in(u, state.c.consts.out_t)
        gt = unet_vjp._reverse(model, state.c, state.tape, gt, state.sizes, sink)
        with_sink = KD.unet_ops.unet_out(gt, state.c.consts.in_t, None, tuple(xi.shape))
    assert torch.equal(with_sink, grad), "the sink changed the activation gradients"
    assert len(sink.grads) == sum(1 for k, _ in model.named_parameters() if k.startswith("u_net.") and "mapper" not in k)    # every conv's

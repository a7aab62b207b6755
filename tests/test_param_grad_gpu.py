"""Parameter gradients and the training loss on the MI355X: the kernels of csrc/wgrad_f32.hip against fp64 on the CPU, ``Denoiser.loss``
and its backward through the HDiT denoiser against fp64 autograd through the CPU oracle, frozen parameters, determinism, the input
gradient's bits, a few optimiser steps followed by a forward through the launch plan, the refusals and a foreign inner model."""
import importlib

import pytest
import torch

from oracle import hdit
from tests.golden import cases
from tests.helpers import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def g(t):
    return t.to(DEV, torch.float32).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bounds(mode, M=1):
    """Kernel bounds against fp64 (max error over the largest entry).  exact: fp32 FMAs, ~1e-6, widening with the rows one chunk sums in
    order (a sum of a few thousand random fp32 terms sits near 1e-6 of the largest entry by itself).  split3: each operand is carried as
    bf16 hi + lo (16 significant bits) and lo x lo is dropped, ~1e-5 per product."""
    return {"exact": 1e-6 if M <= 1024 else 3e-6, "split3": 2e-5}[mode]


# ---------------------------------------------------------------------------------------------------------- kernels

def _gelu_rows(u):
    d = u.shape[-1] // 2
    return u[..., :d] * torch.nn.functional.gelu(u[..., d:])


@pytest.mark.parametrize("M", [1, 3, 37, 4096 + 17, 131072])
@pytest.mark.parametrize("mode", ["exact", "split3"])
def test_wgrad_plain_and_prologues(KD, monkeypatch, M, mode):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    gen = _gen(M)
    # level projections of the shipped configs (qkv, up, down, out at widths 128 .. 512), the mapping network and AdaRMSNorm shapes
    shapes = [(768, 128)] if M == 131072 else [(384, 128), (768, 128), (128, 384), (3072, 512), (1536, 512), (512, 1536), (512, 512),
                                               (1536, 256), (256, 768), (512, 256), (96, 40)]
    for N, K in shapes:
        G, A = torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen)
        ref = G.double().T @ A.double()
        out = KD.ops.wgrad(g(G), g(A))
        assert relerr(out, ref) < _bounds(mode, M), (N, K, relerr(out, ref))
        assert torch.equal(out, KD.ops.wgrad(g(G), g(A)))
        # accumulate + alpha
        base = torch.randn(N, K, generator=gen)
        acc = g(base)
        KD.ops.wgrad(g(G), g(A), out=acc, accumulate=True, alpha=g(torch.tensor([0.75])))
        assert relerr(acc, base.double() + 0.75 * ref) < _bounds(mode, M)
    # the AdaRMSNorm / RMSNorm prologue (row scale, per-sample or shared column scale) and the GEGLU prologue
    N, K = shapes[0]
    B = 1 if M < 4 or M % 2 else 2
    rps = M // B
    G, A = torch.randn(M, N, generator=gen), torch.randn(M, K, generator=gen)
    rr, cs = torch.rand(M, generator=gen) + 0.5, torch.rand(B, K, generator=gen) + 0.5
    ref = G.double().T @ (A.double() * rr.double()[:, None] * cs.double().repeat_interleave(rps, 0))
    out = KD.ops.wgrad(g(G), g(A), row_scale=g(rr), col_scale=g(cs), rows_per_sample=rps)
    assert relerr(out, ref) < _bounds(mode, M), relerr(out, ref)
    ref = G.double().T @ (A.double() * cs[0].double())
    assert relerr(KD.ops.wgrad(g(G), g(A), col_scale=g(cs[0])), ref) < _bounds(mode, M)
    U = torch.randn(M, 2 * K, generator=gen) * 2
    ref = G.double().T @ _gelu_rows(U.double())
    out = KD.ops.wgrad(g(G), g(U), geglu=True)
    assert relerr(out, ref) < _bounds(mode, M), relerr(out, ref)
    assert torch.equal(out, KD.ops.wgrad(g(G), g(U), geglu=True))
    # the arithmetic follows KDIFF_GEMM: split3 on the matrix cores, fp32 FMAs under exact
    other = KD.ops.wgrad(g(G), g(U), geglu=True, precision=KD.ops.nat.PREC_EXACT if mode == "split3" else KD.ops.nat.PREC_SPLIT3)
    assert relerr(other, ref) < _bounds("split3", M)
    if M > 1:
        assert not torch.equal(out, other)


@pytest.mark.parametrize("mode", ["exact", "split3"])
@pytest.mark.parametrize("B,gh,gw,C,N", [(2, 4, 4, 64, 128), (3, 5, 7, 128, 96)])
def test_wgrad_merge_gathers(KD, monkeypatch, mode, B, gh, gw, C, N):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    gen = _gen(gh * gw + C)
    fine = torch.randn(B, 2 * gh, 2 * gw, C, generator=gen)
    merged = fine.view(B, gh, 2, gw, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, 4 * C).double()
    G = torch.randn(B * gh * gw, N, generator=gen)
    out = KD.ops.wgrad(g(G), g(fine), gather=("a", KD.ops.nat.WG_MERGE2x2), gather_geom=(gh, gw, 2, 2, C))
    assert relerr(out, G.double().T @ merged) < _bounds(mode)
    X = torch.randn(B * gh * gw, N, generator=gen)
    out = KD.ops.wgrad(g(fine), g(X), gather=("g", KD.ops.nat.WG_MERGE2x2), gather_geom=(gh, gw, 2, 2, C))
    assert relerr(out, merged.T @ X.double()) < _bounds(mode)


@pytest.mark.parametrize("mode", ["exact", "split3"])
@pytest.mark.parametrize("B,C,H,W,ph", [(2, 3, 16, 16, 2), (3, 1, 28, 28, 4)])
def test_wgrad_patch_gathers(KD, monkeypatch, mode, B, C, H, W, ph):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    gen = _gen(H + C)
    img = torch.randn(B, C, H, W, generator=gen)
    gh, gw = H // ph, W // ph
    patches = img.permute(0, 2, 3, 1).reshape(B, gh, ph, gw, ph, C).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw, ph * ph * C).double()
    G = torch.randn(B * gh * gw, 128, generator=gen)
    out = KD.ops.wgrad(g(G), g(img), gather=("a", KD.ops.nat.WG_PATCH_NCHW), gather_geom=(gh, gw, ph, ph, C))
    assert relerr(out, G.double().T @ patches) < _bounds(mode)
    out = KD.ops.wgrad(g(img), g(G), gather=("g", KD.ops.nat.WG_PATCH_NCHW), gather_geom=(gh, gw, ph, ph, C))
    assert relerr(out, patches.T @ G.double()) < _bounds(mode)


@pytest.mark.parametrize("rows,cols,seg", [(1, 256, 1), (37, 768, 37), (4096 + 16, 128, 2056), (131072, 128, 131072)])
def test_colsum_and_rrms(KD, rows, cols, seg):
    gen = _gen(rows + cols)
    a, b, b2 = (torch.randn(rows, cols, generator=gen) for _ in range(3))
    rs = torch.rand(rows, generator=gen) + 0.5
    prod = a.double() * (b.double() - b2.double()) * rs.double()[:, None]
    ref = prod.view(rows // seg, seg, cols).sum(1)
    out = KD.ops.colsum(g(a), g(b), g(b2), row_scale=g(rs), rows_per_seg=seg)
    assert relerr(out, ref) < 1e-5, relerr(out, ref)
    assert torch.equal(out, KD.ops.colsum(g(a), g(b), g(b2), row_scale=g(rs), rows_per_seg=seg))
    base = torch.randn(rows // seg, cols, generator=gen)
    acc = g(base)
    KD.ops.colsum(g(a), rows_per_seg=seg, out=acc, accumulate=True)
    assert relerr(acc, base.double() + a.double().view(rows // seg, seg, cols).sum(1)) < 1e-5
    rr = KD.ops.row_rrms(g(a))
    assert relerr(rr, torch.rsqrt(a.double().pow(2).mean(-1) + 1e-6)) < 1e-6


def test_attn_scale_and_class_emb_grads(KD):
    gen = _gen(5)
    nh = 4
    cs = torch.randn(3 * nh * 64, generator=gen)
    scale = torch.rand(nh, generator=gen) * 10 + 1
    ref = cs.view(3, nh, 64)[:2].double().sum((0, 2)) / (2 * scale.double())
    assert relerr(KD.ops.attn_scale_grad(g(cs), g(scale), nh), ref) < 1e-6
    gb = torch.randn(7, 256, generator=gen)
    ids = torch.tensor([3, 0, 3, 10, 1, 3, 0])
    ref = torch.zeros(11, 256, dtype=torch.float64).index_add_(0, ids, gb.double())
    out = KD.ops.class_emb_grad(g(gb), ids.to(DEV), 11)
    assert relerr(out, ref) < 1e-6
    assert torch.equal(out, KD.ops.class_emb_grad(g(gb), ids.to(DEV), 11))


def _weight64(kind, sigma, sd):
    if callable(kind):
        return kind(sigma)
    if kind == "karras":
        return torch.ones_like(sigma)
    if kind == "soft-min-snr":
        return (sigma * sd) ** 2 / (sigma ** 2 + sd ** 2) ** 2
    return sd ** 2 / (sigma ** 2 + sd ** 2)


@pytest.mark.parametrize("weighting", ["karras", "soft-min-snr", "snr", "given"])
def test_loss_kernels(KD, weighting):
    gen = _gen(9)
    B, sd = 3, 0.5
    x, n, f = (torch.randn(B, 3, 8, 8, generator=gen) for _ in range(3))
    sigma = torch.tensor([0.05, 1.3, 40.0])
    noised, x_in = KD.ops.loss_prep(g(x), g(n), g(sigma), sd)
    s64 = sigma.double().view(-1, 1, 1, 1)
    nz = x.double() + n.double() * s64
    var = s64 ** 2 + sd ** 2
    assert relerr(noised, nz) < 1e-6 and relerr(x_in, nz / var.sqrt()) < 1e-6
    c_skip, c_out = sd ** 2 / var, s64 * sd / var.sqrt()
    f64 = f.double().requires_grad_()
    given = torch.tensor([0.7, 1.9, 0.05])
    w64 = given.double() if weighting == "given" else _weight64(weighting, sigma.double(), sd)
    cw = g(given) if weighting == "given" else None
    ref = ((f64 - (x.double() - c_skip * nz) / c_out) ** 2).flatten(1).mean(1) * w64
    code = {"karras": 0, "soft-min-snr": 1, "snr": 2, "given": 3}[weighting]
    out = KD.ops.loss(g(f), g(x), noised, g(sigma), sd, code, cw)
    assert relerr(out, ref) < 1e-5, relerr(out, ref)
    gl = torch.tensor([0.3, -1.0, 2.0])
    gf, = torch.autograd.grad(ref, f64, gl.double())
    out = KD.ops.loss_vjp(g(f), g(x), noised, g(sigma), sd, code, g(gl), cw)
    assert relerr(out, gf) < 1e-5, relerr(out, gf)


# ---------------------------------------------------------------------------------------------------------- the model

MC_CFG = {"model": {"type": "image_transformer_v2", "input_channels": 3, "input_size": [16, 16], "patch_size": [2, 2], "depths": [1, 1],
                    "widths": [64, 128], "self_attns": [{"type": "shifted-window", "d_head": 64, "window_size": 4}, {"type": "global", "d_head": 64}],
                    "mapping_cond_dim": 12, "mapping_depth": 1, "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80}}


def _model(KD, name, seed=cases.WEIGHT_SEED):
    """A model of this file's own (the cached models of the other test files stay untouched)."""
    raw = MC_CFG if name == "mapping_cond" else cases.raw_config(name)
    cfg = KD.config.load_config(raw)
    model = KD.config.make_model(cfg).eval()
    sd = KD.synth.synth_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd)
    return cfg, model.to(DEV), sd


def _inputs(cfg, batch, seed=41):
    mc = cfg["model"]
    gen = _gen(seed)
    x = torch.randn(batch, mc["input_channels"], *mc["input_size"], generator=gen) * 0.5
    noise = torch.randn(x.shape, generator=gen)
    sigma = torch.tensor([0.3, 6.0, 1.1, 25.0][:batch])
    nc = cases.num_classes_of(cfg)
    kw = {}
    if nc:
        kw["class_cond"] = (torch.arange(batch) * 3 + 1) % (nc + 1)
    if mc.get("mapping_cond_dim", 0):
        kw["mapping_cond"] = torch.randn(batch, mc["mapping_cond_dim"], generator=gen)
        kw["aug_cond"] = torch.randn(batch, 9, generator=gen) * 0.3
    return x, noise, sigma, kw


def _oracle_loss(cfg, model, sd, x, noise, sigma, kw, weighting="karras"):
    """(losses, {name: gradient}) of mean(losses) under fp64 autograd through oracle.hdit.forward."""
    mc = cfg["model"]
    names = {n for n, _ in model.named_parameters()}
    torch.set_default_dtype(torch.float64)
    try:
        sd64 = {k: (v.double().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
        kw64 = {k: (v.double() if v.is_floating_point() else v) for k, v in kw.items()}
        sdata = mc["sigma_data"]
        s64 = sigma.double()
        var = (s64 ** 2 + sdata ** 2).view(-1, 1, 1, 1)
        c_skip, c_out, c_in = sdata ** 2 / var, s64.view(-1, 1, 1, 1) * sdata / var.sqrt(), 1 / var.sqrt()
        noised = x.double() + noise.double() * s64.view(-1, 1, 1, 1)
        f = hdit.forward(sd64, mc, noised * c_in, s64, **kw64)
        target = (x.double() - c_skip * noised) / c_out
        losses = ((f - target) ** 2).flatten(1).mean(1) * _weight64(weighting, s64, sdata)
        grads = torch.autograd.grad(losses.mean(), [sd64[n] for n in sorted(names)])
    finally:
        torch.set_default_dtype(torch.float32)
    return losses.detach(), dict(zip(sorted(names), grads))


def _hip_loss(KD, model, cfg, x, noise, sigma, kw, weighting="karras"):
    model.zero_grad(set_to_none=True)
    den = KD.Denoiser(model, cfg["model"]["sigma_data"], weighting=weighting)
    losses = den.loss(g(x), g(noise), g(sigma), **{k: v.to(DEV) for k, v in kw.items()})
    losses.mean().backward()
    return losses.detach(), {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("name,batch", [("tiny_global", 2), ("tiny_sw", 2), ("tiny_na", 2), ("tiny_odd", 2), ("mapping_cond", 2),
                                        ("mnist", 1), ("cifar", 1)])
@pytest.mark.parametrize("mode,tol", [("exact", 1e-4), ("split3", 3e-4)])
def test_parameter_gradients_vs_oracle(KD, monkeypatch, name, batch, mode, tol):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    cfg, model, sd = _model(KD, name)
    x, noise, sigma, kw = _inputs(cfg, batch)
    ref_l, ref_g = _oracle_loss(cfg, model, sd, x, noise, sigma, kw)
    got_l, got_g = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    assert (got_l.cpu().double() - ref_l).abs().max() / ref_l.abs().max() < 1e-5, (got_l, ref_l)
    misses = {}
    for n, ref in ref_g.items():
        assert got_g[n] is not None, f"{n}: no gradient"
        e = relerr(got_g[n], ref)
        if not e < tol:
            misses[n] = e
    assert not misses, misses


@pytest.mark.parametrize("weighting", ["soft-min-snr", "snr", "callable"])
def test_loss_weightings(KD, weighting):
    cfg, model, sd = _model(KD, "tiny_sw")
    x, noise, sigma, kw = _inputs(cfg, 2)
    sdata = cfg["model"]["sigma_data"]
    w = (lambda s: 1.0 / (s + 1.0)) if weighting == "callable" else weighting
    ref_l, _ = _oracle_loss(cfg, model, sd, x, noise, sigma, kw, weighting="karras")
    ref_l = ref_l * (1.0 / (sigma.double() + 1.0) if weighting == "callable" else _weight64(weighting, sigma.double(), sdata))
    with torch.no_grad():
        got = KD.Denoiser(model, sdata, weighting=w).loss(g(x), g(noise), g(sigma), **{k: v.to(DEV) for k, v in kw.items()})
    assert ((got.cpu().double() - ref_l).abs() / ref_l.abs()).max() < 1e-5, (got, ref_l)
    if weighting == "callable":                     # the given-weight gradient (kd_loss_vjp_f32, KD_LW_GIVEN) through the model
        _, ref_g = _oracle_loss(cfg, model, sd, x, noise, sigma, kw, weighting=lambda s: 1.0 / (s + 1.0))
        _, got_g = _hip_loss(KD, model, cfg, x, noise, sigma, kw, weighting=w)
        misses = {n: relerr(got_g[n], r) for n, r in ref_g.items() if not relerr(got_g[n], r) < 3e-4}
        assert not misses, misses


def test_frozen_subset_and_determinism(KD):
    cfg, model, _ = _model(KD, "tiny_sw")
    x, noise, sigma, kw = _inputs(cfg, 2)
    _, full = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    full = {n: t.clone() for n, t in full.items()}
    _, again = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    for n in full:
        assert torch.equal(full[n], again[n]), n
    frozen = {n for i, (n, _) in enumerate(model.named_parameters()) if i % 3 != 1}
    for n, p in model.named_parameters():
        p.requires_grad_(n not in frozen)
    _, part = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    for n in full:
        if n in frozen:
            assert part[n] is None, n
        else:
            assert torch.equal(part[n], full[n]), n
    # only the last layer's projections trainable: the walk skips the rest and gives the same bits
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("patch_out."))
    _, last = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    assert torch.equal(last["patch_out.proj.weight"], full["patch_out.proj.weight"])
    assert sum(t is not None for t in last.values()) == 1


def test_input_gradient_route_is_bit_identical(KD):
    vjp = importlib.import_module(KD.__name__ + ".models.vjp")
    cfg, model, _ = _model(KD, "tiny_na")
    x, _, sigma, kw = _inputs(cfg, 2)
    gx = g(x).requires_grad_()
    out = model(gx, g(sigma))
    gout = torch.randn(out.shape, generator=_gen(3)).to(DEV)
    out.backward(gout)
    gx2, grads = vjp.backward(model, g(x), g(sigma), gout, params=list(model.parameters()))
    assert torch.equal(gx.grad, gx2)
    assert len(grads) == len(list(model.parameters()))
    assert all(p.grad is None for p in model.parameters())


def test_train_then_sample(KD):
    cfg, model, _ = _model(KD, "tiny_sw")
    mc = cfg["model"]
    x, noise, sigma, kw = _inputs(cfg, 4)
    kw = {k: v.to(DEV) for k, v in kw.items()}
    den = KD.Denoiser(model, mc["sigma_data"])
    opt = torch.optim.AdamW(model.param_groups(2e-3), betas=(0.9, 0.99))
    # a forward through the launch plan before training: the plan must follow the in-place updates
    with torch.no_grad():
        den(g(x), g(sigma), **kw)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = den.loss(g(x), g(noise), g(sigma), **kw).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    fresh = KD.config.make_model(cfg).eval()
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(DEV)
    with torch.no_grad():
        a = den(g(x), g(sigma), **kw)
        b = KD.Denoiser(fresh, mc["sigma_data"])(g(x), g(sigma), **kw)
    assert torch.equal(a, b)


def test_refusals(KD):
    cfg, model, _ = _model(KD, "tiny_global")
    x, noise, sigma, _ = _inputs(cfg, 2)
    den = KD.Denoiser(model, 0.5)
    for i, name in enumerate(("input", "noise", "sigma")):
        args = [g(x), g(noise), g(sigma)]
        args[i].requires_grad_()
        with pytest.raises(NotImplementedError, match=f"w.r.t. {name}.*{name}.detach"):
            den.loss(*args)
    with pytest.raises(NotImplementedError, match="aug_cond"):
        den.loss(g(x), g(noise), g(sigma), aug_cond=torch.zeros(2, 9, device=DEV, requires_grad=True))
    with pytest.raises(NotImplementedError, match="scales"):
        KD.Denoiser(model, 0.5, scales=2).loss(g(x), g(noise), g(sigma))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.loss(x, noise, sigma)
    raw = cases.raw_config("tiny_global")
    raw["model"]["dropout_rate"] = 0.1
    mdrop = KD.config.make_model(KD.config.load_config(raw)).to(DEV)
    with pytest.raises(NotImplementedError, match=r"dropout.*model\.eval\(\)"):
        KD.Denoiser(mdrop, 0.5).loss(g(x), g(noise), g(sigma))
    KD.Denoiser(mdrop.eval(), 0.5).loss(g(x), g(noise), g(sigma)).mean().backward()
    for cls in (KD.layers.DenoiserWithVariance, KD.layers.SimpleLossDenoiser):
        with pytest.raises(NotImplementedError):
            cls(model, 0.5).loss(g(x), g(noise), g(sigma))


def test_foreign_inner_model(KD):
    class Small(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 3, 3, padding=1)
            self.lin = torch.nn.Linear(1, 3)

        def forward(self, x, sigma):
            return self.conv(x) * torch.tanh(self.lin(sigma.log()[:, None] / 4))[:, :, None, None]
    torch.manual_seed(0)
    inner = Small()
    inner64 = Small().double()
    inner64.load_state_dict(inner.state_dict())
    inner = inner.to(DEV)
    gen = _gen(2)
    x, noise = torch.randn(2, 3, 8, 8, generator=gen), torch.randn(2, 3, 8, 8, generator=gen)
    sigma = torch.tensor([0.4, 3.0])
    losses = KD.Denoiser(inner, 0.5, weighting="snr").loss(g(x), g(noise), g(sigma))
    losses.sum().backward()
    s64 = sigma.double().view(-1, 1, 1, 1)
    var = s64 ** 2 + 0.25
    nz = x.double() + noise.double() * s64
    f = inner64(nz / var.sqrt(), sigma.double())
    ref = ((f - (x.double() - 0.25 / var * nz) / (s64 * 0.5 / var.sqrt())) ** 2).flatten(1).mean(1) * (0.25 / (sigma.double() ** 2 + 0.25))
    ref.sum().backward()
    assert relerr(losses, ref) < 1e-5
    for (n, p), (_, p64) in zip(inner.named_parameters(), inner64.named_parameters()):
        assert relerr(p.grad, p64.grad) < 1e-4, n

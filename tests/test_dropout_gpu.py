"""Dropout in the training loss on the MI355X: the mask kernels against a numpy restatement of the mask contract (include/kdiff_hip.h),
the fused GEGLU VJP and weight-gradient prologue against their unfused forms and fp64, ``Denoiser.loss`` with dropout and every parameter
gradient against fp64 autograd through the CPU oracle with the same masks injected, reproducibility, the bits when dropout is off, the
refusals and a few optimiser steps with dropout."""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hdit
from oracle.brownian import philox4x32_10
from tests.golden import cases
from tests.helpers import relerr
from tests.test_param_grad_gpu import MC_CFG, _bounds, _gelu_rows, _hip_loss, _inputs, _oracle_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
SITES = [(1 << 62) | 5, (1 << 62) | (1 << 32) | 1]
KEYS = [-3, 0x0123456789ABCDEF]


def g(t):
    return t.to(DEV, torch.float32).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _key(k):
    return torch.tensor([k], dtype=torch.int64, device=DEV)


def np_mask(key, site, p, n):
    """The mask contract restated: element e keeps iff word e & 3 of philox4x32_10(key, e >> 2, site) >= floor(p 2^32); kept elements
    are multiplied by (float)(1 / (1 - p)), dropped ones by 0.  Returns the float32 multipliers."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(key & (2 ** 64 - 1), q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), site & 0xFFFFFFFF, site >> 32)
    w = np.stack(np.broadcast_arrays(*words), axis=1).reshape(-1)[:n]
    keep = w >= np.uint32(int(np.floor(p * 2.0 ** 32)))
    return np.where(keep, np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------- mask kernels

@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2 ** 20 + 3])
def test_dropout_matches_the_contract(KD, n):
    x = torch.randn(n, generator=_gen(n)) * 3
    xn = x.numpy()
    for key in KEYS:
        for site in SITES:
            for p in (0.05, 0.1, 0.5, 0.9):
                ref = (xn * np_mask(key, site, p, n)).astype(np.float32)
                y = KD.ops.dropout(g(x), _key(key), site, p)
                assert np.array_equal(_bits(y), ref.view(np.uint32)), (key, site, p)
                if n == 1027 and p == 0.5:
                    z = g(x)
                    assert KD.ops.dropout(z, _key(key), site, p, out=z) is z
                    assert torch.equal(z, y)                                        # in place == out of place
                    sub = g(x)[1:]                                                  # not 16-byte aligned: the element loop
                    ref1 = (xn[1:] * np_mask(key, site, p, n - 1)).astype(np.float32)
                    assert np.array_equal(_bits(KD.ops.dropout(sub, _key(key), site, p)), ref1.view(np.uint32))
    xg = g(x)
    assert KD.ops.dropout(xg, _key(1), SITES[0], 0.0) is xg                       # p == 0: nothing launched


def test_dropout_nan_inf_and_refusals(KD):
    n = 4096
    x = torch.randn(n, generator=_gen(1))
    x[::7] = float("nan")
    x[3::14] = float("inf")
    with np.errstate(invalid="ignore"):
        ref = x.numpy() * np_mask(KEYS[1], SITES[0], 0.5, n)
    y = KD.ops.dropout(g(x), _key(KEYS[1]), SITES[0], 0.5).cpu().numpy()
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    assert np.isnan(y[::7]).all()
    fin = ~np.isnan(ref)
    assert np.array_equal(y[fin], ref[fin])
    for p in (1.0, -0.1):
        with pytest.raises(ValueError, match="outside"):
            KD.ops.dropout(g(x), _key(1), SITES[0], p)


@pytest.mark.parametrize("p", [0.05, 0.5, 0.9])
def test_dropout_statistics(KD, p):
    n = 2 ** 22
    ones = torch.ones(n, device=DEV)
    k = _key(KEYS[1])
    a = KD.ops.dropout(ones, k, SITES[0], p) != 0
    b = KD.ops.dropout(ones, k, SITES[1], p) != 0
    frac = a.double().mean().item()
    assert abs(frac - (1 - p)) < 6 * (p * (1 - p) / n) ** 0.5, frac
    q = (1 - p) ** 2 + p ** 2
    agree = (a == b).double().mean().item()
    assert abs(agree - q) < 6 * (q * (1 - q) / n) ** 0.5, agree


# ---------------------------------------------------------------------------------------------------------- fused kernels

@pytest.mark.parametrize("rows,d_ff", [(1, 4), (5, 3), (37, 768), (1024, 1536)])
def test_geglu_vjp_drop_is_the_unfused_pair(KD, rows, d_ff):
    gen = _gen(rows + d_ff)
    u, gy = g(torch.randn(rows, 2 * d_ff, generator=gen) * 2), g(torch.randn(rows, d_ff, generator=gen))
    k = _key(KEYS[0])
    for p in (0.1, 0.5):
        fused = KD.ops.geglu_vjp(u, gy, dropout=(k, SITES[0], p))
        pair = KD.ops.geglu_vjp(u, KD.ops.dropout(gy, k, SITES[0], p))
        assert torch.equal(fused, pair), p
    assert torch.equal(KD.ops.geglu_vjp(u, gy, dropout=(k, SITES[0], 0.0)), KD.ops.geglu_vjp(u, gy))


def _wgrad_drop_raw(KD, G, U, key, site, threshold, scale, split3):
    """kd_wgrad_drop_f32 called directly (GEGLU prologue, plain operands)."""
    nat = KD.ops.nat
    M, N = G.shape
    K = U.shape[1] // 2
    chunk, nchunk = KD.ops.wgrad_chunks(M, N, K)
    ws = torch.empty(nchunk * N * K, device=DEV)
    out = torch.empty(N, K, device=DEV)
    bits = torch.empty((M * K + 31) // 32, device=DEV, dtype=torch.int32)
    p = KD.ops._p
    nat.check(nat.lib().kd_wgrad_drop_f32(p(G), 0, p(U), 0, 1, M, N, K, 0, 0, 0, 0, 0, None, None, 0, 1, None, 0, int(split3), chunk, nchunk,
                                           p(ws), p(out), p(key), site, threshold, scale, p(bits), KD.ops._stream()), "kd_wgrad_drop_f32")
    return out


@pytest.mark.parametrize("M", [3, 37, 4096 + 17])
@pytest.mark.parametrize("mode", ["exact", "split3"])
def test_wgrad_drop_vs_fp64(KD, monkeypatch, M, mode):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    gen = _gen(M)
    N, K = 128, 384
    G, U = torch.randn(M, N, generator=gen), torch.randn(M, 2 * K, generator=gen) * 2
    k = _key(KEYS[1])
    for p in (0.1, 0.5):
        mask = KD.ops.dropout(torch.ones(M, K, device=DEV), k, SITES[0], p)
        assert np.array_equal(_bits(mask).reshape(-1), np_mask(KEYS[1], SITES[0], p, M * K).view(np.uint32))
        ref = G.double().T @ (mask.cpu().double() * _gelu_rows(U.double()))
        out = KD.ops.wgrad(g(G), g(U), geglu=True, dropout=(k, SITES[0], p))
        assert relerr(out, ref) < _bounds(mode, M), (p, relerr(out, ref))
        assert torch.equal(out, KD.ops.wgrad(g(G), g(U), geglu=True, dropout=(k, SITES[0], p)))
        A = torch.randn(M, K, generator=gen)                                         # a plain A operand under the mask
        ref = G.double().T @ (mask.cpu().double() * A.double())
        assert relerr(KD.ops.wgrad(g(G), g(A), dropout=(k, SITES[0], p)), ref) < _bounds(mode, M)
    # p == 0: today's bits, through ops and through the entry point itself (threshold 0)
    plain = KD.ops.wgrad(g(G), g(U), geglu=True)
    assert torch.equal(KD.ops.wgrad(g(G), g(U), geglu=True, dropout=(k, SITES[0], 0.0)), plain)
    assert torch.equal(_wgrad_drop_raw(KD, g(G), g(U), k, SITES[0], 0, 1.0, mode == "split3"), plain)


# ---------------------------------------------------------------------------------------------------------- the model against the oracle

SHIPPED_RATES = {"mnist": 0.05, "cifar": 0.05}                # the reference's configs (the JSON files here do not carry them)


def _itv2(KD):
    return importlib.import_module(KD.__name__ + ".models.image_transformer_v2")


def _drop_model(KD, name, rate=None, mapping_rate=None, seed=cases.WEIGHT_SEED):
    """(cfg, model in training mode on the device, CPU state dict) with the given dropout rates."""
    raw = copy.deepcopy(MC_CFG) if name == "mapping_cond" else cases.raw_config(name)
    if rate is not None:
        raw["model"]["dropout_rate"] = rate
    if mapping_rate is not None:
        raw["model"]["mapping_dropout_rate"] = mapping_rate
    cfg = KD.config.load_config(raw)
    model = KD.config.make_model(cfg)
    sd = KD.synth.synth_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd)
    return cfg, model.to(DEV).train(), sd


def _site_masks(KD, model, x, key):
    """{(oracle prefix, kind) or ("mapping", k): fp64 mask} of every dropout site of ``model`` under ``key``, made by ``ops.dropout`` on
    ones and checked against the numpy restatement first."""
    grids = model._token_grids(g(x))
    B = x.shape[0]
    kt = _key(key)
    out = {}
    for site, where, kind, p in _itv2(KD).dropout_sites(model):
        if kind == "mapping":
            shape, name = (B, model.mapping_spec.d_ff), ("mapping", where)
        else:
            gh, gw = grids[where.level]
            spec = model.level_specs[where.level]
            shape = (B, gh, gw, spec.width if kind == "attn" else spec.d_ff)
            name = (where.prefix + ("self_attn." if kind == "attn" else "ff."), kind)
        m = KD.ops.dropout(torch.ones(shape, device=DEV), kt, site, p)
        assert np.array_equal(_bits(m).reshape(-1), np_mask(key, site, p, m.numel()).view(np.uint32)), name
        out[name] = m.cpu().double()
    return out


def _patch_oracle(monkeypatch, masks):
    """oracle.hdit with the masks at the reference's dropout sites (the oracle's own files stay as they are)."""
    def self_attention_block(sd, prefix, spec, layer_index, x, pos, cond):
        skip = x
        n_heads = x.shape[-1] // spec.get("d_head", 64)
        qkv = hdit.norm_linear(x, cond, sd[prefix + "norm.linear.weight"], sd[prefix + "qkv_proj.weight"])
        q, k, v = hdit.split_qkv(qkv, n_heads)
        q, k = hdit.cosine_sim_scale(q, k, sd[prefix + "scale"])
        theta = hdit.rope_theta(pos, sd[prefix + "pos_emb.freqs"])
        q, k = hdit.apply_rope(q, theta), hdit.apply_rope(k, theta)
        kind = spec["type"]
        if kind == "global":
            o = hdit.attn_global(q, k, v, 1.0)
        elif kind == "neighborhood":
            o = hdit.na2d(q, k, v, spec.get("kernel_size", 7), 1.0)
        else:
            ws = spec["window_size"]
            o = hdit.attn_shifted_window(q, k, v, ws, ws // 2 if layer_index % 2 == 1 else 0, 1.0)
        o = o.reshape(*o.shape[:3], -1)
        m = masks.get((prefix, "attn"))
        return (o if m is None else o * m) @ sd[prefix + "out_proj.weight"].T + skip

    def feed_forward_block(sd, prefix, x, cond):
        h = hdit.norm_linear(x, cond, sd[prefix + "norm.linear.weight"], sd[prefix + "up_proj.weight"])
        d = h.shape[-1] // 2
        h = h[..., :d] * F.gelu(h[..., d:])
        m = masks.get((prefix, "ff"))
        return (h if m is None else h * m) @ sd[prefix + "down_proj.weight"].T + x

    def mapping_network(sd, x, depth):
        x = hdit.rms_norm(x, sd["mapping.in_norm.scale"])
        for i in range(depth):
            p = f"mapping.blocks.{i}."
            h = hdit.linear_geglu(hdit.rms_norm(x, sd[p + "norm.scale"]), sd[p + "up_proj.weight"])
            m = masks.get(("mapping", i))
            x = (h if m is None else h * m) @ sd[p + "down_proj.weight"].T + x
        return hdit.rms_norm(x, sd["mapping.out_norm.scale"])

    monkeypatch.setattr(hdit, "self_attention_block", self_attention_block)
    monkeypatch.setattr(hdit, "feed_forward_block", feed_forward_block)
    monkeypatch.setattr(hdit, "mapping_network", mapping_network)


def _replay_key(seed):
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, device=DEV,
                             generator=torch.Generator(DEV).manual_seed(seed)).item())


@pytest.mark.parametrize("name,batch,rate,mrate", [("tiny_global", 2, 0.2, None), ("tiny_sw", 2, 0.3, None), ("tiny_na", 2, [0.25, 0.0, 0.2], None),
                                                   ("tiny_odd", 2, 0.25, None), ("mapping_cond", 2, 0.2, 0.2),
                                                   ("mnist", 1, SHIPPED_RATES["mnist"], None), ("cifar", 1, SHIPPED_RATES["cifar"], None)])
@pytest.mark.parametrize("mode,tol", [("exact", 1e-4), ("split3", 3e-4)])
def test_dropout_gradients_vs_oracle(KD, monkeypatch, name, batch, rate, mrate, mode, tol):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    cfg, model, sd = _drop_model(KD, name, rate, mrate)
    x, noise, sigma, kw = _inputs(cfg, batch)
    seed = 1234 + batch
    model.enable_dropout(torch.Generator(DEV).manual_seed(seed))
    got_l, got_g = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    masks = _site_masks(KD, model, x, _replay_key(seed))
    assert masks and any(m.eq(0).any() for m in masks.values())
    if mrate:
        assert ("mapping", 0) in masks
    _patch_oracle(monkeypatch, masks)
    ref_l, ref_g = _oracle_loss(cfg, model, sd, x, noise, sigma, kw)
    assert (got_l.cpu().double() - ref_l).abs().max() / ref_l.abs().max() < 1e-5, (got_l, ref_l)
    misses = {}
    for n, ref in ref_g.items():
        assert got_g[n] is not None, f"{n}: no gradient"
        e = relerr(got_g[n], ref)
        if not e < tol:
            misses[n] = e
    assert not misses, misses


# ---------------------------------------------------------------------------------------------------------- reproducibility, off

def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)


def test_reproducible_and_fresh_keys(KD):
    cfg, model, _ = _drop_model(KD, "tiny_sw", 0.2)
    x, noise, sigma, kw = _inputs(cfg, 2)
    gen = torch.Generator(DEV)
    model.enable_dropout(gen)
    gen.manual_seed(7)
    l1, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    g1 = _grads(model)
    l2, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)                     # the next call draws a new key
    assert not torch.equal(l1, l2)
    gen.manual_seed(7)
    l3, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    assert torch.equal(l1, l3) and _same(g1, _grads(model))
    # no generator: torch's default generator of the device, governed by torch.manual_seed
    model.enable_dropout()
    torch.manual_seed(7)
    l4, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    assert torch.equal(l4, l1)
    # the same key under no_grad gives the same losses
    gen.manual_seed(7)
    model.enable_dropout(gen)
    with torch.no_grad():
        l5 = KD.Denoiser(model, cfg["model"]["sigma_data"]).loss(g(x), g(noise), g(sigma), **{k: v.to(DEV) for k, v in kw.items()})
    assert torch.equal(l5, l1)


def test_off_is_todays_bits(KD):
    cfg, model, _ = _drop_model(KD, "tiny_sw", 0.2)
    x, noise, sigma, kw = _inputs(cfg, 2)
    model.eval()
    base_l, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)                 # not enabled, eval()
    base_g = _grads(model)
    gen = torch.Generator(DEV).manual_seed(3)
    state = gen.get_state()
    model.enable_dropout(gen)                                                   # enabled, eval()
    l1, _ = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    assert torch.equal(l1, base_l) and _same(_grads(model), base_g)
    cfg0, model0, _ = _drop_model(KD, "tiny_sw", 0.0)                          # enabled, training mode, every rate 0
    model0.enable_dropout(gen)
    l0, _ = _hip_loss(KD, model0, cfg0, x, noise, sigma, kw)
    assert torch.equal(l0, base_l) and _same(_grads(model0), base_g)
    assert torch.equal(gen.get_state(), state)                                  # nothing drawn


def test_frozen_subset_same_key(KD):
    cfg, model, _ = _drop_model(KD, "tiny_sw", 0.2)
    x, noise, sigma, kw = _inputs(cfg, 2)
    gen = torch.Generator(DEV)
    model.enable_dropout(gen)
    gen.manual_seed(11)
    _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    full = _grads(model)
    frozen = {n for i, (n, _) in enumerate(model.named_parameters()) if i % 3 != 1}
    for n, p in model.named_parameters():
        p.requires_grad_(n not in frozen)
    gen.manual_seed(11)
    _, part = _hip_loss(KD, model, cfg, x, noise, sigma, kw)
    for n in full:
        if n in frozen:
            assert part[n] is None, n
        else:
            assert torch.equal(part[n], full[n]), n


# ---------------------------------------------------------------------------------------------------------- refusals

def test_refusals(KD):
    cfg, model, _ = _drop_model(KD, "tiny_global", 0.1)
    x, noise, sigma, _ = _inputs(cfg, 2)
    xs, ss = g(x), g(sigma)
    model(xs, ss)                                   # not enabled: forward runs in training mode as before
    with pytest.raises(NotImplementedError, match=r"dropout.*model\.eval\(\)"):
        KD.Denoiser(model, 0.5).loss(xs, g(noise), ss)
    model.enable_dropout()
    for call in (lambda: model(xs, ss), lambda: model.forward_preconditioned(xs, ss, 0.5), lambda: model.forward_jvp(xs, ss, torch.ones_like(xs))):
        with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
            call()
    model.eval()
    model(xs, ss)
    model.forward_preconditioned(xs, ss, 0.5)
    model.forward_jvp(xs, ss, torch.ones_like(xs))
    for bad in (1.0, -0.1):
        _, mb, _ = _drop_model(KD, "tiny_global", bad)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            mb.enable_dropout()


# ---------------------------------------------------------------------------------------------------------- training

def test_train_with_dropout_then_sample(KD):
    cfg, model, _ = _drop_model(KD, "tiny_sw", 0.1)
    mc = cfg["model"]
    x, noise, sigma, kw = _inputs(cfg, 4)
    kw = {k: v.to(DEV) for k, v in kw.items()}
    den = KD.Denoiser(model, mc["sigma_data"])
    model.enable_dropout(torch.Generator(DEV).manual_seed(5))
    opt = torch.optim.AdamW(model.param_groups(2e-3), betas=(0.9, 0.99))
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = den.loss(g(x), g(noise), g(sigma), **kw).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    model.eval()
    fresh = KD.config.make_model(cfg).eval()
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    fresh = fresh.to(DEV)
    with torch.no_grad():
        a = den(g(x), g(sigma), **kw)
        b = KD.Denoiser(fresh, mc["sigma_data"])(g(x), g(sigma), **kw)
    assert torch.equal(a, b)

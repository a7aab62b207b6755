"""Level 0 of the 256 x 256 neighbourhood configs in the fp32-parity (split3) mode: neighbourhood attention core + out projection +
residual + feed-forward block as ONE launch (kd_attn_ffn_f32, csrc/attn_ffn_x3.hip) against the two launches it replaces
(kd_attn_na2d_f32, then kd_ffn_f32 with the fused out projection).  Every product keeps its term and accumulation order, so the
gate is torch.equal: on the kernel's own output, on a whole forward and on a sampler run (plan switch KDIFF_ATTN_FFN).
Needs a real MI355X:  pytest -m gpu."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = 7

_model = {}


def flowers(KD):
    if not _model:
        cfg = KD.config.load_config(json.load(open(os.path.join(REPO, "configs", "config_oxford_flowers.json"))))
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(KD.synth.synth_state_dict(model.state_dict(), seed=7))
        _model["m"] = (cfg, model.to(DEV))
    return _model["m"]


def noise(KD, shape, seed, scale):
    """[shape[0], ...] seeded fp32 values (K.synth's per-sample generator)."""
    return KD.synth.synth_noise_batch(tuple(shape[1:]), seed, 0, shape[0], scale)


@pytest.mark.parametrize("batch", [1, 3, 32])
def test_fused_launch_gives_the_two_launches_bits(KD, monkeypatch, batch):
    """Level 0 of config_oxford_flowers.json (64 x 64 tokens, width 128, 2 heads, kernel 7) with the model's own layer-0 weights: the new
    residual stream of the one launch equals the two launches' bit for bit -- every tile of every sample, border tiles (clamped
    windows) included -- out of place and in place (as the model runs it)."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    from k_diffusion_amd import ops
    cfg, model = flowers(KD)
    lv = model.level_specs[0]
    (H, W), (ph, pw) = cfg["model"]["input_size"], model.patch_size
    gh, gw, d, nh = H // ph, W // pw, lv.width, lv.width // lv.self_attn.d_head
    assert (gh, gw, d, nh, lv.self_attn.kernel_size) == (64, 64, 128, 2, KS)
    assert ops.attn_ffn_supported(batch, gh, gw, nh, KS, d, lv.d_ff)
    layer = model.down_levels[0][0]
    wo, wu, wd = layer.self_attn.out_proj.weight, layer.ff.up_proj.weight, layer.ff.down_proj.weight
    q, k, v = (noise(KD, (batch, gh, gw, nh, 64), s, sc) for s, sc in ((101, 0.5), (102, 0.5), (103, 1.0)))
    qkv = torch.stack([KD.compat._split_stored(t) for t in (q, k, v)], dim=3).reshape(batch, gh, gw, 3 * nh * 64).contiguous().to(DEV)
    x = noise(KD, (batch, gh, gw, d), 104, 1.0).to(DEV)
    scale = (1 + 0.2 * noise(KD, (batch, d), 105, 1.0)).to(DEV)
    att = ops.attn_na2d(qkv, nh, KS, prep="packed")
    two = ops.ffn(x, scale, wu, wd, rows_per_sample=gh * gw, attn=att.view(batch, gh, gw, d), w_out=wo)
    one = ops.attn_ffn(qkv, nh, KS, x, scale, wu, wd, wo)
    torch.cuda.synchronize()
    assert torch.isfinite(two).all() and not torch.equal(two, x)
    bad = (one != two).any(dim=-1)
    print(f"batch {batch}: {int(bad.sum())} of {bad.numel()} rows differ, max abs diff {(one - two).abs().max().item():.3e}")
    assert torch.equal(one, two)
    border = torch.ones(gh, gw, dtype=torch.bool)
    border[KS // 2:gh - KS // 2, KS // 2:gw - KS // 2] = False
    assert torch.equal(one[:, border], two[:, border])                 # the rows whose window is clamped
    xi = x.clone()
    ops.attn_ffn(qkv, nh, KS, xi, scale, wu, wd, wo, out=xi)
    assert torch.equal(xi, two)


def test_shapes_outside_level_0_keep_the_two_launches(KD, monkeypatch):
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    from k_diffusion_amd import ops
    assert not ops.attn_ffn_supported(4, 60, 64, 2, KS, 128, 256)       # token grid not a multiple of the 8 x 16 tile
    assert not ops.attn_ffn_supported(4, 64, 64, 2, 5, 128, 256)        # another kernel size
    assert not ops.attn_ffn_supported(4, 32, 32, 4, KS, 256, 768)       # width 256
    assert not ops.attn_ffn_supported(2, 16, 16, 2, KS, 128, 256)       # fewer rows than the fused FF kernel takes
    x = torch.zeros(1, 60, 64, 128, device=DEV)
    with pytest.raises(RuntimeError, match="kd_attn_ffn_f32"):
        ops.attn_ffn(torch.zeros(1, 60, 64, 384, device=DEV), 2, KS, x, torch.ones(1, 128, device=DEV), torch.zeros(512, 128, device=DEV),
                     torch.zeros(128, 256, device=DEV), torch.zeros(128, 128, device=DEV))


def _plan(KD, model, batch, flag):
    names = [n for n, _ in KD.models.image_transformer_v2.PLAN_SWITCHES]
    found = [p for key, p in model._plans.items() if key[0] == batch and key[7] == KD._native.PREC_SPLIT3 and key[8 + names.index("KDIFF_ATTN_FFN")] == flag]
    assert found, flag
    return found[-1]


def test_forward_and_sampler_with_the_switch_on_and_off(KD, monkeypatch):
    """A whole forward and a 5-step DPM++2M run: KDIFF_ATTN_FFN=1 (default; the level-0 layers are one launch each) against =0."""
    monkeypatch.setenv("KDIFF_GEMM", "split3")
    from tests.golden import cases
    cfg, model = flowers(KD)
    mc, batch = cfg["model"], 4
    x, sigma, cls = cases.forward_inputs(cfg, batch, cases.b32_sigmas(batch))
    kw = {"class_cond": cls.to(DEV)} if cls is not None else {}
    sig = KD.sampling.get_sigmas_karras(5, mc["sigma_min"], mc["sigma_max"], device=DEV)
    x0 = KD.synth.synth_noise_batch(tuple(x.shape[1:]), 3, 0, batch, mc["sigma_max"]).to(DEV)
    fwd, smp, names = {}, {}, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("KDIFF_ATTN_FFN", flag)
        fwd[flag] = model(x.to(DEV), sigma.to(DEV), **kw).clone()
        names[flag] = [ln.what for ln in _plan(KD, model, batch, flag).launches]
        smp[flag] = KD.sampling.sample_dpmpp_2m(KD.Denoiser(model, mc["sigma_data"]), x0.clone(), sig, extra_args=kw, disable=True).clone()
    torch.cuda.synchronize()
    fused = [n for n in names["1"] if n.endswith("attn_na2d+ff")]
    depth0 = len(model.down_levels[0]) + len(model.up_levels[0])
    assert len(fused) == depth0 and not any(n.endswith("+ff") for n in names["0"])
    assert len(names["0"]) - len(names["1"]) == depth0                  # one launch less per level-0 layer
    assert torch.isfinite(fwd["0"]).all() and torch.isfinite(smp["0"]).all()
    print(f"forward max abs diff {(fwd['1'] - fwd['0']).abs().max().item():.3e}, sampler {(smp['1'] - smp['0']).abs().max().item():.3e}")
    assert torch.equal(fwd["1"], fwd["0"])
    assert torch.equal(smp["1"], smp["0"])

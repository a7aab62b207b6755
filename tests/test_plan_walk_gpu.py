"""The bf16 and fp8 launch plans against an op-by-op walk of the same network on the same kernels (tests/plan_walk.py): BIT equality.

The model-level gates of these two modes are sized to their arithmetic noise (2e-2 .. 3e-2 in bf16, ~9e-2 and more in fp8: tests/test_model_gpu.py),
so a wiring mistake of the plan that costs a few per cent -- an AdaRMSNorm reading another norm's slice of the scale table, the hidden
activation's scale bytes at the wrong offset of ``hid``, a window shift from the wrong layer index, ``rows_per_sample`` of the wrong level, a
split's skip from the wrong buffer -- passes them.  The walker issues one public ``ops`` call per launch of the plan, on fresh tensors, with the
routes ``route_layer`` gives the plan: same entry points, same shapes, same operand values, so ``torch.equal`` must hold, and any wiring
difference changes bits.  Equality would also hold if both shared a mistake through ``ops`` or ``route_layer``, so the walker itself is held
against the CPU oracle at the project's existing bf16 / fp8 forward gates (``test_walker_*_vs_oracle``).

Every case asserts the launch forms it is there for, so that its coverage cannot disappear silently when a threshold moves.
profiles/plan_wiring_tests.md: which one-line mutation of the plan each test catches, and the wall time of this file.
"""
import pytest
import torch

from oracle import hdit
from tests.golden import cases
from tests.helpers import relerr
from tests.plan_walk import walk
from tests.test_model_gpu import FP8_FLOOR, FP8_NOISE_FACTOR

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHT_SEED = 31
MAPPING_COND_DIM = 12

G = {"type": "global", "d_head": 64}
SW8 = {"type": "shifted-window", "d_head": 64, "window_size": 8}
NA7 = {"type": "neighborhood", "d_head": 64, "kernel_size": 7}


def _raw(depths, widths, d_ffs, attns, num_classes=0, mapping_cond_dim=0):
    raw = {"model": {"type": "image_transformer_v2", "input_channels": 3, "input_size": [64, 64], "patch_size": [2, 2], "depths": depths,
                     "widths": widths, "d_ffs": d_ffs, "self_attns": attns, "mapping_cond_dim": mapping_cond_dim, "sigma_data": 0.5,
                     "sigma_min": 1e-2, "sigma_max": 80}}
    if num_classes:
        raw["dataset"] = {"num_classes": num_classes}
    return raw


def _wire3(level0, depth0=2):
    return _raw([depth0, 2, 2], [128, 256, 512], [384, 704, 1536], [level0, G, G], num_classes=5, mapping_cond_dim=MAPPING_COND_DIM)


CONFIGS = {
    "cifar": lambda: cases.raw_config("cifar"),
    # three levels: 32 x 32 tokens at width 128 (local attention), 16 x 16 at width 256 / d_ff 704, 8 x 8 at width 512 / d_ff 1536
    "wire3_sw": lambda: _wire3(SW8),
    "wire3_na": lambda: _wire3(NA7),
    # as wire3_sw with ONE layer per side at level 0: the down layer has index 0 (no shift), the up layer index 1 (shift 4).  At depth 2 an up
    # layer's index i + depth has the parity of i, so a plan that forgot the offset would compute the same windows there
    "wire3_sw1": lambda: _wire3(SW8, depth0=1),
    # two levels, 24 576 rows at level 0 at batch 24: the block-form projections of the bf16 mode
    "wire_block": lambda: _raw([2, 2], [256, 512], [384, 1536], [NA7, G]),
}
# wire3: the fp8 projections from 128 rows on, and the fused FF block (width 128, with its fused out projection) from 8 192 rows on instead of
# the default 16 384 -- level 0 has 1 024 tokens per sample, so batch 8 takes the fused block and batches 2 and 3 the up / down pair
WIRE3_OPTIONS = "mx8_min_rows=128,ffn_bf16_min_rows=8192"

_models, _oracle = {}, {}


def _build(KD, name):
    if name not in _models:
        cfg = KD.config.load_config(CONFIGS[name]())
        model = KD.config.make_model(cfg).eval().requires_grad_(False)
        model.load_state_dict(KD.synth.synth_state_dict(model.state_dict(), seed=WEIGHT_SEED))
        _models[name] = (cfg, model.to(DEV))
    return _models[name]


def _inputs(cfg, batch, aug, top=None, seed=17):
    """Seeded inputs of the first ``batch`` samples of a ``top``-sample draw (CPU tensors): x at every sample's own sigma, and the conditioning
    the config asks for; ``aug``: a real aug_cond, else the constant path."""
    top = top or batch
    m = cfg["model"]
    g = torch.Generator().manual_seed(seed)
    sigma = (torch.rand(top, generator=g) * 7 - 3).exp()
    x = torch.randn(top, m["input_channels"], *m["input_size"], generator=g) * (sigma.view(-1, 1, 1, 1) ** 2 + 0.25).sqrt()
    aug_cond, mapping_cond = torch.randn(top, 9, generator=g) * 0.4, torch.randn(top, MAPPING_COND_DIM, generator=g)
    kw = {}
    nc = cases.num_classes_of(cfg)
    if nc:
        kw["class_cond"] = ((torch.arange(top) * 3 + 1) % (nc + 1))[:batch].contiguous()         # includes the "uncond" id nc
    if m["mapping_cond_dim"]:
        kw["mapping_cond"] = mapping_cond[:batch].contiguous()
    if aug:
        kw["aug_cond"] = aug_cond[:batch].contiguous()
    return x[:batch].contiguous(), sigma[:batch].contiguous(), kw


def _per_sample(a, b):
    """Max-norm relative error of every sample."""
    a, b = a.detach().float().flatten(1), b.detach().float().flatten(1)
    return ((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30)).tolist()


def _set_mode(monkeypatch, mode, options):
    monkeypatch.setenv("KDIFF_GEMM", mode)
    if options:
        monkeypatch.setenv("KDIFF_OPTIONS", options)
    else:
        monkeypatch.delenv("KDIFF_OPTIONS", raising=False)


def _plan_equals_walk(KD, monkeypatch, name, mode, batch, options=None, aug=False, top=None):
    """Asserts plan == walker (bits) for ``model(x, sigma, ...)`` and for ``Denoiser(model, sigma_data)(...)``; returns (the plan's launch names,
    the denoiser's output)."""
    _set_mode(monkeypatch, mode, options)
    cfg, model = _build(KD, name)
    x, sigma, kw = _inputs(cfg, batch, aug, top)
    x, sigma, kw = x.to(DEV), sigma.to(DEV), {k: v.to(DEV) for k, v in kw.items()}
    sigma_data = cfg["model"]["sigma_data"]
    den = KD.Denoiser(model, sigma_data)
    got = None
    for what, sd in (("model", None), ("Denoiser", sigma_data)):
        got = model(x, sigma, **kw) if sd is None else den(x, sigma, **kw)
        plan = list(model._plans.values())[-1]                  # (most recently used last)
        assert plan.B == batch and plan.mode == {"bf16": KD._native.PREC_BF16, "fp8": KD._native.PREC_FP8}[mode]
        streams = {}
        want = walk(model, x, sigma, mode=mode, sigma_data=sd, streams=streams, **kw)
        assert torch.isfinite(want).all()
        if not torch.equal(got, want):
            # localisation only: the levels' final residual streams, as the plan's run left them
            print(f"{name} [{mode}] batch {batch}, {what}: plan != walker; per sample {['%.3e' % e for e in _per_sample(got, want)]}")
            for li, s in sorted(streams.items()):
                print(f"  level {li} final residual stream: per sample {['%.3e' % e for e in _per_sample(plan.xs[li], s)]}")
        assert torch.equal(got, want), (name, mode, batch, what)
    return [ln.what for ln in plan.launches], got


def _layers(KD, model):
    """(prefix, level, heads) of every layer, forward order."""
    v2 = KD.models.image_transformer_v2
    return [(st.prefix, st.level, model.level_specs[st.level].width // 64) for st in v2.hourglass(model) if st.kind == "layer"]


# ---- (a) CIFAR-10 config, both levels on the fp8 projections at batch 2: level 1 has exactly 128 rows, the kernel's minimum -----------------

@pytest.mark.parametrize("aug", [False, True], ids=["aug_const", "aug_cond"])
@pytest.mark.parametrize("mode", ["fp8", "bf16"])
def test_cifar_batch2_plan_equals_walk(KD, monkeypatch, mode, aug):
    names, _ = _plan_equals_walk(KD, monkeypatch, "cifar", mode, 2, options="mx8_min_rows=128", aug=aug)
    _, model = _build(KD, "cifar")
    for prefix, _, _ in _layers(KD, model):
        mx8 = "(mx8)" if mode == "fp8" else ""
        want = [prefix + "qkv_proj" + mx8, prefix + "attn_global", prefix + "out_proj", prefix + "up_proj" + mx8, prefix + "down_proj" + mx8]
        assert [w for w in names if w.startswith(prefix)] == want


# ---- (b) CIFAR-10 config, fp8 at the default mx8_min_rows: both sides of the 4 096-row threshold of either level ----------------------------

THRESHOLD_BATCHES = (15, 16, 17, 63, 64)
TOKENS = {0: 256, 1: 64}             # per sample and level: level 0 reaches 4 096 rows at batch 16, level 1 at batch 64
_threshold_out = {}


@pytest.mark.parametrize("batch", THRESHOLD_BATCHES)
def test_cifar_fp8_default_threshold_plan_equals_walk(KD, monkeypatch, batch):
    names, out = _plan_equals_walk(KD, monkeypatch, "cifar", "fp8", batch, top=max(THRESHOLD_BATCHES))
    _threshold_out[batch] = out[0].cpu()
    _, model = _build(KD, "cifar")
    level_mx8 = {0: False, 1: False}
    for prefix, li, nh in _layers(KD, model):
        mine = [w for w in names if w.startswith(prefix)]
        expect = batch * TOKENS[li] >= 4096
        level_mx8[li] |= any(w.endswith("(mx8)") for w in mine)
        block = prefix + "attn_block" in mine
        if block:                    # the plan prefers the one-launch bf16 attention block from 32 (sample, head) problems on
            assert TOKENS[li] == 256 and batch * nh >= 32 and prefix + "qkv_proj(mx8)" not in mine and prefix + "qkv_proj" not in mine
        else:
            assert (prefix + "qkv_proj(mx8)" in mine) == expect and (prefix + "qkv_proj" in mine) == (not expect), (prefix, mine)
        for proj in ("up_proj", "down_proj"):
            assert (prefix + proj + "(mx8)" in mine) == expect and (prefix + proj in mine) == (not expect), (prefix, mine)
        assert any(w.endswith("(mx8)") for w in mine) == expect, (prefix, mine)
    # both sides of both thresholds are really there
    assert level_mx8 == {0: batch >= 16, 1: batch >= 64}


def test_cifar_fp8_sample_0_across_the_threshold(KD, monkeypatch):
    """The loose statement across the threshold: sample 0 in a batch of 15 (level 0 on the bf16 projections) against the same sample in a batch
    of 16 (level 0 on the fp8 ones), at the per-sample fp8 gate of test_batch_sizes_between_the_tested_ones_agree_across_modes.  The tight
    statement is plan == walker on either side (above)."""
    for batch in (15, 16):
        if batch not in _threshold_out:
            _threshold_out[batch] = _plan_equals_walk(KD, monkeypatch, "cifar", "fp8", batch, top=max(THRESHOLD_BATCHES))[1][0].cpu()
    e = _per_sample(_threshold_out[15][None], _threshold_out[16][None])[0]
    print(f"cifar [fp8] sample 0, batch 15 against batch 16: {e:.3e}")
    assert e < 2.5e-1


# ---- (c) wire3: three levels, every conditioning input, ragged panels ----------------------------------------------------------------------

def _wire3_expected(name, mode, batch):
    """Launch names a wire3 case must contain, and names it must not."""
    mx8 = "(mx8)" if mode == "fp8" else ""
    core0 = "attn_window" if name.startswith("wire3_sw") else "attn_na2d"
    need, never = [], []
    for p in ("down_levels.0.0.", "up_levels.0.0."):
        need.append(p + core0)
        if batch >= 8:               # 8 192 rows: the fused width-128 FF block with the out projection in front of it
            need.append(p + "ff")
            never += [p + "out_proj", p + "up_proj", p + "down_proj"]
        else:
            need += [p + "qkv_proj", p + "out_proj", p + "up_proj", p + "down_proj"]
            never.append(p + "ff")
    for p in ("down_levels.1.0.", "up_levels.1.1."):
        if batch >= 8:               # 32 (sample, head) problems: the one-launch attention block
            need.append(p + "attn_block")
            never += [p + "qkv_proj" + mx8, p + "attn_global"]
        else:
            need += [p + "qkv_proj" + mx8, p + "attn_global"]
            never.append(p + "attn_block")
        need += [p + "out_proj", p + "up_proj" + mx8, p + "down_proj"]          # d_ff = 704: the down projection stays bf16 on a bf16 `hid`
        never.append(p + "down_proj(mx8)")
    for p in ("mid_level.0.", "mid_level.1."):                                   # d_ff = 1536: e4m3 `hid` + scale bytes
        need += [p + "qkv_proj" + mx8, p + "attn_global", p + "out_proj", p + "up_proj" + mx8, p + "down_proj" + mx8]
    need += ["merges.0", "merges.1", "splits.1", "splits.0", "patch_in", "patch_out"]
    return need, never


@pytest.mark.parametrize("batch", [2, 3, 8])
@pytest.mark.parametrize("mode", ["fp8", "bf16"])
@pytest.mark.parametrize("name", ["wire3_sw", "wire3_na"])
def test_wire3_plan_equals_walk(KD, monkeypatch, name, mode, batch):
    """Batch 3: level 2 has 192 rows, a ragged 128-row panel; a real aug_cond at batches 2 and 8, the constant path at batch 3."""
    names, _ = _plan_equals_walk(KD, monkeypatch, name, mode, batch, options=WIRE3_OPTIONS, aug=batch != 3)
    need, never = _wire3_expected(name, mode, batch)
    assert not [w for w in need if w not in names] and not [w for w in never if w in names], names


@pytest.mark.parametrize("mode", ["fp8", "bf16"])
def test_wire3_odd_depth_window_shift_plan_equals_walk(KD, monkeypatch, mode):
    """One shifted-window layer per side at level 0: the up layer's shift (index 1) differs from the down layer's (index 0)."""
    names, _ = _plan_equals_walk(KD, monkeypatch, "wire3_sw1", mode, 2, options=WIRE3_OPTIONS, aug=True)
    assert "down_levels.0.0.attn_window" in names and "up_levels.0.0.attn_window" in names
    _, model = _build(KD, "wire3_sw1")
    v2 = KD.models.image_transformer_v2
    shifts = [v2.attn_geometry(model.level_specs[0].self_attn, st.index)[2][1] for st in v2.hourglass(model) if st.kind == "layer" and st.level == 0]
    assert shifts == [0, 4]


# ---- (d) wire_block: the block-form projections of the bf16 mode, which the fp8 mode replaces -----------------------------------------------

@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_wire_block_plan_equals_walk(KD, monkeypatch, mode):
    names, _ = _plan_equals_walk(KD, monkeypatch, "wire_block", mode, 24)
    for p in ("down_levels.0.0.", "down_levels.0.1.", "up_levels.0.0.", "up_levels.0.1."):
        mine = [w for w in names if w.startswith(p)]
        if mode == "bf16":           # 24 576 rows: 192 workgroups in the block form
            assert mine == [p + "qkv_proj(block)", p + "attn_na2d", p + "out_proj", p + "up_proj(block)", p + "down_proj"]
        else:                        # at the default threshold the same layers go to the fp8 instruction (d_ff = 384: a bf16 down projection)
            assert mine == [p + "qkv_proj(mx8)", p + "attn_na2d", p + "out_proj", p + "up_proj(mx8)", p + "down_proj"]
    for p in ("mid_level.0.", "mid_level.1."):
        assert p + "attn_block" in names and p + ("up_proj(block)" if mode == "bf16" else "up_proj(mx8)") in names


# ---- the walker itself against the CPU oracle ----------------------------------------------------------------------------------------------

def _oracle_refs(KD, name):
    """(fp32 statement, mx8 statement) of the oracle for the batch-2 inputs of ``name``, computed once."""
    if name not in _oracle:
        cfg, model = _build(KD, name)
        x, sigma, kw = _inputs(cfg, 2, True)
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref32 = hdit.forward(sd, cfg["model"], x, sigma, **kw)
        with hdit.mx8_arithmetic():
            ref8 = hdit.forward(sd, cfg["model"], x, sigma, **kw)
        _oracle[name] = (ref32, ref8)
    return _oracle[name]


def _walk_batch2(KD, monkeypatch, name, mode):
    _set_mode(monkeypatch, mode, WIRE3_OPTIONS)
    cfg, model = _build(KD, name)
    x, sigma, kw = _inputs(cfg, 2, True)
    return walk(model, x.to(DEV), sigma.to(DEV), mode=mode, **{k: v.to(DEV) for k, v in kw.items()})


@pytest.mark.parametrize("name", ["wire3_sw", "wire3_na", "wire3_sw1"])
def test_walker_bf16_vs_oracle(KD, monkeypatch, name):
    """The bf16 forward gate of test_unusual_shapes_bf16 (2.5e-2 against the fp32 CPU oracle)."""
    e = relerr(_walk_batch2(KD, monkeypatch, name, "bf16"), _oracle_refs(KD, name)[0])
    print(f"{name}: walker [bf16] vs fp32 oracle {e:.3e}")
    assert e < 2.5e-2


@pytest.mark.parametrize("name", ["wire3_sw", "wire3_na", "wire3_sw1"])
def test_walker_fp8_vs_oracle(KD, monkeypatch, name):
    """The fp8 forward gate of test_forward_fp8_mode against the oracle's restatement of the kernel's arithmetic: FP8_NOISE_FACTOR x the
    distance between the oracle's mx8 statement and its fp32 statement on the same weights, never below FP8_FLOOR."""
    ref32, ref8 = _oracle_refs(KD, name)
    got = _walk_batch2(KD, monkeypatch, name, "fp8")
    e, own = relerr(got, ref8), relerr(ref8, ref32)
    print(f"{name}: walker [fp8] vs the oracle's mx8 statement {e:.3e} (that statement vs the oracle's fp32 one: {own:.3e})")
    assert e < max(FP8_NOISE_FACTOR * own, FP8_FLOOR)

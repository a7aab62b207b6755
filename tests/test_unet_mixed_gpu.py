"""bf16 weight-gradient arithmetic of the image_v1 U-Net on the MI355X, and the family on the command line: the convolution weight-gradient
kernel ``kd_conv2d_wgrad_bf16`` (csrc/conv_wgrad_bf16.hip; ``unet_ops.conv2d_wgrad(bf16=True)``), ``set_wgrad_arithmetic("bf16")`` on the bare
and the wrapped model, and ``train.py`` on image_v1 configs end to end.

Bounds.
* exact cases (integer operands in -4 .. 4; one-hot taps; ties and near-ties): ``torch.equal`` -- every product and sum is exact in fp32, and
  the rounding is ``torch.Tensor.bfloat16()``'s.
* random normals: truth is fp64 ``conv2d_weight`` of the operands rounded by ``.bfloat16()`` on the CPU, the yardstick the same call in fp32 on
  the CPU; ``max|hip - truth| <= max(4 max|yard - truth|, 2^-21 max|truth|)`` -- the project's 4 x convention (tests/test_wgrad_bf16_gpu.py,
  tests/test_training_gpu.py) and a floor of four fp32 ulps of the result for the 2 x 2 shape whose yardstick is one ulp.  The split kernel on
  the same UNROUNDED operands must miss that bound: the test tells the two arithmetics apart.
* model: the loss bit-equal to the default's; per parameter ``relerr <= max(err_ref[param], 5e-4)`` against fp64 autograd over the restated
  loss, err_ref the REAL reference's own bf16-autocast error (tests/golden/unet_wgrad_bf16.json), 5e-4 the family's split3 gate.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import unet_ref as ur
from tests import unet_train_ref as tr
from tests.test_unet_gpu import DEV, g, rel, rn, tokens
from tests.test_unet_train_cpu import restated
from tests.test_unet_train_gpu import WGRAD_CASES, _operand, grads_of, hip_loss, profiled, trainable, wgrad_reference

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT3_GATE = 5e-4
SHAPES = sorted({case[:5] for case in WGRAD_CASES})


def _patches(B, hw):
    return B * -(-hw[0] // 8) * -(-hw[1] // 8)


def _two_chunks(B, hw):
    patches = _patches(B, hw)
    return -(-patches // 2), 2 if patches > 1 else 1                   # one patch cannot be cut in two


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def integer_reference(B, hw, ci, co, ks):
    """(a, g, dW in fp64) with integer-valued operands in -4 .. 4: every product and every partial sum is an integer below 2^24."""
    H, W = hw
    gen = torch.Generator().manual_seed(3 * ci + 5 * H + W)
    a = torch.randint(-4, 5, (B, ci, H, W), generator=gen).float()
    gy = torch.randint(-4, 5, (B, co, H, W), generator=gen).float()
    ref = torch.nn.grad.conv2d_weight(a.double(), (co, ci, ks, ks), gy.double(), padding=ks // 2)
    assert B * H * W * 16 < 2 ** 24
    return a, gy, ref


@pytest.mark.parametrize("B,hw,ci,co,ks,layout", WGRAD_CASES, ids=str)
def test_conv_wgrad_bf16_indexes_exactly(KD, B, hw, ci, co, ks, layout):
    uo = KD.unet_ops
    a, gy, ref = integer_reference(B, hw, ci, co, ks)
    at, gt = _operand(tokens(a), layout, "a"), _operand(tokens(gy), layout, "g")
    dw = uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=True)
    assert dw.shape == (co, ci, ks, ks) and torch.equal(dw.cpu().double(), ref), "the default chunking"
    other = uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=True, chunks=_two_chunks(B, hw))
    assert torch.equal(other.cpu().double(), ref), "two chunks"


@pytest.mark.parametrize("ks", [3, 1])
def test_conv_wgrad_bf16_one_hot_lights_one_tap(KD, ks):
    """A one-hot pixel / channel in A and in G lights exactly one (co, ci, ky, kx): a flipped or transposed tap shows."""
    uo = KD.unet_ops
    B, H, W, ci, co = 2, 9, 11, 128, 64
    taps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] if ks == 3 else [(0, 0)]
    for n, (dy, dx) in enumerate(taps):
        b, y, x, c_a, c_g = n % B, 8 if dy < 0 else 7, 8 + (n % 2), (37 + 5 * n) % ci, (11 + 3 * n) % co      # across the patch boundary at 8
        a, gy = torch.zeros(B, H, W, ci), torch.zeros(B, H, W, co)
        gy[b, y, x, c_g] = 2.0
        a[b, y + dy, x + dx, c_a] = 0.75                                 # G[y, x] meets A[y + ky - h, x + kx - h]: ky = dy + h
        dw = uo.conv2d_wgrad(g(gy.reshape(-1, co)), g(a.reshape(-1, ci)), B, H, W, ks, bf16=True).cpu()
        want = torch.zeros(co, ci, ks, ks)
        want[c_g, c_a, dy + ks // 2, dx + ks // 2] = 1.5
        assert torch.equal(dw, want), f"tap ({dy}, {dx}): lit {dw.nonzero().tolist()}, expected {want.nonzero().tolist()}"
    # the same pixel in another sample does not meet it
    a, gy = torch.zeros(B, H, W, ci), torch.zeros(B, H, W, co)
    gy[0, 4, 4, 1], a[1, 4, 4, 2] = 1.0, 1.0
    assert not bool(uo.conv2d_wgrad(g(gy.reshape(-1, co)), g(a.reshape(-1, ci)), B, H, W, ks, bf16=True).any())


@pytest.mark.parametrize("ks", [3, 1])
def test_conv_wgrad_bf16_rounds_to_nearest_even(KD, ks):
    """A one-hot G = 1 copies A into the lit taps, rounded: ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), near-ties (1 + 2^-8 + 2^-20 ->
    1 + 2^-7) and their negatives come out as ``A.bfloat16()``, bit for bit -- nearest even, and no lo part."""
    uo = KD.unet_ops
    B, H, W, ci, co = 2, 9, 11, 128, 64
    vals = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])
    vals = torch.cat([vals, -vals])
    assert vals.bfloat16().float().tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, -(1 + 2.0 ** -6), -(1 + 2.0 ** -7)]
    a = vals[(torch.arange(B * H * W * ci) * 7 // 3) % 6].reshape(B, H, W, ci)
    b, y, x, c_g, h = 1, 7, 8, 13, ks // 2                             # the neighbourhood crosses the patch boundary at 8, inside the image
    gy = torch.zeros(B, H, W, co)
    gy[b, y, x, c_g] = 1.0
    dw = uo.conv2d_wgrad(g(gy.reshape(-1, co)), g(a.reshape(-1, ci)), B, H, W, ks, bf16=True).cpu()
    want = torch.zeros(co, ci, ks, ks)
    for ky in range(ks):
        for kx in range(ks):
            want[c_g, :, ky, kx] = a[b, y + ky - h, x + kx - h].bfloat16().float()
    assert torch.equal(dw, want)
    assert not torch.equal(want[c_g], a[b, y - h:y + h + 1, x - h:x + h + 1].permute(2, 0, 1)), "the pattern holds nothing to round"


@functools.lru_cache(maxsize=None)
def rounded_reference(B, hw, ci, co, ks):
    """(a, g, truth, bound): the unrounded operands of ``wgrad_reference``; truth = fp64 ``conv2d_weight`` of the operands rounded by
    ``.bfloat16()``; bound = max(4 max|yard - truth|, 2^-21 max|truth|), yard the same call in fp32 on the CPU."""
    a, gy, _ = wgrad_reference(B, hw, ci, co, ks)
    ab, gb = a.bfloat16(), gy.bfloat16()
    truth = torch.nn.grad.conv2d_weight(ab.double(), (co, ci, ks, ks), gb.double(), padding=ks // 2)
    yard = torch.nn.grad.conv2d_weight(ab.float(), (co, ci, ks, ks), gb.float(), padding=ks // 2)
    e_yard = (yard.double() - truth).abs().max().item()
    return a, gy, truth, max(4 * e_yard, 2.0 ** -21 * truth.abs().max().item()), e_yard


@pytest.mark.parametrize("B,hw,ci,co,ks,layout", WGRAD_CASES, ids=str)
def test_conv_wgrad_bf16_random_normals(KD, B, hw, ci, co, ks, layout):
    """Measured (error / yardstick, MI355X): see DESIGN.md section 8."""
    uo = KD.unet_ops
    a, gy, truth, bound, e_yard = rounded_reference(B, hw, ci, co, ks)
    at, gt = _operand(tokens(a), layout, "a"), _operand(tokens(gy), layout, "g")
    per, n = uo.conv_wgrad_chunks(B, *hw, ci, co)
    (dw, names) = profiled(KD._native, lambda: uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=True))
    err = (dw.cpu().double() - truth).abs().max().item()
    split = uo.conv2d_wgrad(gt, at, B, *hw, ks)
    e_split = (split.cpu().double() - truth).abs().max().item()
    one = uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=True, chunks=(_patches(B, hw), 1))
    e_one = (one.cpu().double() - truth).abs().max().item()
    e_yard = max(e_yard, 1e-300)                                      # (printed ratios only; the bound has its floor)
    print(f"conv wgrad bf16 B{B} {hw[0]}x{hw[1]} {ci}->{co} k{ks} {layout}: error {err:.3e} = {err / e_yard:.2f} x the yardstick {e_yard:.3e} "
          f"(bound {bound:.3e} = {bound / e_yard:.1f} x); one chunk {e_one / e_yard:.2f} x; the split kernel on the unrounded operands "
          f"{e_split / e_yard:.0f} x; {n} chunk(s) of {per} patches; {names}")
    assert dw.shape == (co, ci, ks, ks)
    assert err <= bound
    assert e_one <= bound
    assert not e_split <= bound, "the bound cannot tell bf16 operands from unrounded ones"
    assert any(nm.startswith(f"conv2d_wgrad_bf16<k{ks}>") and nm.endswith(f" chunks={n}") for nm in names), names
    assert not any(nm.startswith("conv2d_wgrad_x3") for nm in names), names
    assert torch.equal(uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=True), dw), "a repeat gives other bits"
    # accumulate: one fp32 addition to what out holds
    acc0 = g(rn(co, ci, ks, ks, seed=5))
    acc = uo.conv2d_wgrad(gt, at, B, *hw, ks, out=acc0.clone(), accumulate=True, bf16=True)
    assert torch.equal(acc, acc0 + dw)
    # the folded 1 / 8 of a qkv projection's q rows: exact
    q = uo.conv2d_wgrad(gt, at, B, *hw, ks, q_rows=64, bf16=True)
    assert torch.equal(q[:64], dw[:64] * 0.125) and torch.equal(q[64:], dw[64:])


def test_conv_wgrad_bf16_refuses_what_it_does_not_take(KD):
    uo = KD.unet_ops
    gt, at = g(rn(2 * 16, 64)), g(rn(2 * 16, 64, seed=1))
    with pytest.raises(RuntimeError, match="kd_conv2d_wgrad_bf16.*multiples of 64"):
        uo.conv2d_wgrad(g(rn(32, 96)), at, 2, 4, 4, 3, bf16=True)
    with pytest.raises(RuntimeError, match="kd_conv2d_wgrad_bf16.*kernel size"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 5, bf16=True)
    with pytest.raises(RuntimeError, match="kd_conv2d_wgrad_bf16.*do not cut"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 3, chunks=(1, 3), bf16=True)
    with pytest.raises(ValueError, match="rows for batch"):
        uo.conv2d_wgrad(gt, at, 2, 4, 5, 3, bf16=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uo.conv2d_wgrad(gt.cpu(), at, 2, 4, 4, 3, bf16=True)
    with pytest.raises(ValueError, match="accumulate needs"):
        uo.conv2d_wgrad(gt, at, 2, 4, 4, 3, accumulate=True, bf16=True)


@pytest.mark.parametrize("B,hw,ci,co,ks", SHAPES, ids=str)
def test_the_default_path_keeps_its_bits(KD, B, hw, ci, co, ks):
    uo = KD.unet_ops
    a, gy, _ = wgrad_reference(B, hw, ci, co, ks)
    at, gt = g(tokens(a)), g(tokens(gy))
    (off, names) = profiled(KD._native, lambda: uo.conv2d_wgrad(gt, at, B, *hw, ks, bf16=False))
    assert torch.equal(off, uo.conv2d_wgrad(gt, at, B, *hw, ks))
    assert any(nm.startswith(f"conv2d_wgrad_x3<k{ks}>") for nm in names) and not any("wgrad_bf16" in nm for nm in names), names


# ---- 2. the model --------------------------------------------------------------------------------------------------------------------------------

WEIGHTINGS = ("karras", "soft-min-snr")


def _err_ref(name, weighting):
    return json.load(open(os.path.join(REPO, "tests", "golden", "unet_wgrad_bf16.json")))[name][weighting]


def _loss_and_grads(KD, model, name, weighting):
    model.zero_grad(set_to_none=True)
    losses = hip_loss(KD, model, name, weighting)
    losses.mean().backward()
    return losses.detach().clone(), {k: v.clone() for k, v in grads_of(model).items()}


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_model_gradients_within_the_references_bf16_error(KD, name, weighting):
    """Measured (worst error / bound per config and weighting, and how many gradients moved): see DESIGN.md section 8."""
    err_ref = _err_ref(name, weighting)
    _, want = restated(name, weighting)
    model = trainable(KD, name)
    loss0, g0 = _loss_and_grads(KD, model, name, weighting)
    assert model.set_wgrad_arithmetic("bf16") is model
    loss1, g1 = _loss_and_grads(KD, model, name, weighting)
    assert torch.equal(loss0, loss1), "the primal moved"
    params = dict(model.named_parameters())
    assert sorted(g1) == sorted(want) == sorted(err_ref)
    worst_k, worst_r, misses = "", 0.0, {}
    for k, ref in want.items():
        e, bound = rel(g1[k], ref), max(err_ref[k], SPLIT3_GATE)
        if e / bound > worst_r:
            worst_k, worst_r = k, e / bound
        if not e <= bound:
            misses[k] = (e, bound)
    moved = sorted(k for k in g0 if not torch.equal(g0[k], g1[k]))
    weights = sorted(k for k, p in params.items() if k.endswith(".weight") and p.dim() >= 2)
    print(f"{name} {weighting}: worst error / bound {worst_r:.3f} ({worst_k}); {len(moved)} of {len(g0)} gradients moved")
    assert not misses, misses
    assert moved == weights, "every convolution and Linear weight moves, and no bias"
    assert len(moved) == {"unet_a": 44, "unet_b": 38}[name] and not any(k.endswith(".bias") for k in moved)
    # switched off again: the default's bits, which are a fresh model's
    assert model.set_wgrad_arithmetic(None) is model
    _, g2 = _loss_and_grads(KD, model, name, weighting)
    _, g3 = _loss_and_grads(KD, trainable(KD, name), name, weighting)
    for k in g0:
        assert torch.equal(g2[k], g0[k]) and torch.equal(g3[k], g0[k]), k


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_vjp_keeps_its_bits(KD, name):
    model = trainable(KD, name).requires_grad_(False)
    x, _, sigma, aug = tr.batch(name)
    kw = {} if aug is None else {"aug_cond": g(aug)}
    u = g(rn(*x.shape, seed=29))
    out0, pull0 = model.forward_vjp(g(x), g(sigma), **kw)
    gx0 = pull0(u)
    model.set_wgrad_arithmetic("bf16")
    out1, pull1 = model.forward_vjp(g(x), g(sigma), **kw)
    assert torch.equal(out0, out1) and torch.equal(gx0, pull1(u))


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_under_dropout_only_the_weight_products_move(KD, name):
    """Dropout at 0.25 with the same seed: the masks, the loss and every bias keep their bits; a 3 x 3 weight's gradient differs from the split3
    run's by the window of tests/test_wgrad_bf16_gpu.py::test_bf16_request_is_honoured_under_exact -- bf16 operands: far from fp32-grade,
    close to the gradient."""
    from tests.test_unet_drop_gpu import dropping, seeded
    runs = {}
    for arithmetic in (None, "bf16"):
        model = dropping(KD, name, 0.25)
        seeded(model, 7)
        model.set_wgrad_arithmetic(arithmetic)
        runs[arithmetic] = _loss_and_grads(KD, model, name, "karras")
        params = dict(model.named_parameters())
    (loss0, g0), (loss1, g1) = runs[None], runs["bf16"]
    assert torch.equal(loss0, loss1)
    biases = [k for k in g0 if k.endswith(".bias")]
    assert biases and any("mapper" in k for k in biases) and all(torch.equal(g0[k], g1[k]) for k in biases)
    convs = [k for k, p in params.items() if p.dim() == 4 and p.shape[2] == 3]
    errs = {k: rel(g1[k], g0[k].cpu()) for k in convs}
    print(f"{name}: {len(convs)} 3x3 weights, bf16 against split3 under dropout: {min(errs.values()):.2e} .. {max(errs.values()):.2e}")
    assert convs and all(1e-5 < e < 2e-2 for e in errs.values()), errs


# ---- 3. train.py ---------------------------------------------------------------------------------------------------------------------------------

def _run_train(cwd, args, timeout=420):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


TAIL = {"optimizer": {"type": "adamw", "lr": 5e-4, "betas": [0.9, 0.95], "eps": 1e-8, "weight_decay": 1e-3},
        "lr_sched": {"type": "constant", "warmup": 0.0}, "ema_sched": {"type": "inverse", "power": 0.75, "max_value": 0.9999}}


def _unet_config(dataset, **model):
    base = {"type": "image_v1", "input_channels": 3, "input_size": [16, 16], "patch_size": 1, "mapping_out": 64, "depths": [1, 1],
            "channels": [64, 128], "self_attn_depths": [False, True], "has_variance": False, "loss_config": "karras",
            "loss_weighting": "soft-min-snr", "dropout_rate": 0.05, "augment_wrapper": True, "augment_prob": 0.12, "sigma_data": 0.5,
            "sigma_min": 1e-2, "sigma_max": 80, "sigma_sample_density": {"type": "cosine-interpolated"}}
    return dict(TAIL, model=dict(base, **model), dataset=dataset)


@pytest.fixture()
def image_folder(tmp_path):
    from PIL import Image
    data_dir = tmp_path / "images"
    data_dir.mkdir()
    gen = torch.Generator().manual_seed(8)
    for i in range(16):
        arr = (torch.rand(16, 16, 3, generator=gen) * 255).to(torch.uint8).numpy()
        Image.fromarray(arr, mode="RGB").save(data_dir / f"img_{i:02}.png")
    return data_dir


def test_train_py_wrapped_unet_end_to_end(KD, tmp_path, image_folder):
    """The reference's U-Net recipe in small: the augmentation wrapper, dropout 0.05, augment_prob 0.12 on the device, soft-min-snr,
    gradient accumulation, checkpoints, a demo grid, and a bit-exact ``--resume``."""
    from PIL import Image
    config = _unet_config({"type": "imagefolder", "location": str(image_folder)})
    (tmp_path / "config.json").write_text(json.dumps(config))
    common = ["--config", str(tmp_path / "config.json"), "--device-augment", "--batch-size", "4", "--grad-accum-steps", "2", "--save-every", "3",
              "--demo-every", "6", "--sample-n", "4", "--seed", "1", "--num-workers", "0"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    out = _run_train(a, [*common, "--end-step", "6", "--name", "run"])
    assert "Device augmentation: a_prob 0.12" in out.stdout and "Mixed precision" not in out.stdout
    for f in ("run_00000003.pth", "run_00000006.pth", "run_state.json", "run_log.csv", "run_demo_00000006.png"):
        assert (a / f).exists(), f
    assert json.load(open(a / "run_state.json")) == {"latest_checkpoint": "run_00000006.pth"}
    assert len((a / "run_log.csv").read_text().strip().splitlines()) == 7
    assert Image.open(a / "run_demo_00000006.png").size == (32, 32)
    full = torch.load(a / "run_00000006.pth", map_location="cpu", weights_only=False)
    assert {"model", "model_ema", "opt", "sched", "ema_sched", "epoch", "step", "gns_stats", "ema_stats"} <= set(full)
    assert full["step"] == 6 and full["gns_stats"] is None and full["ema_sched"]["last_epoch"] == 3
    assert all(k.startswith("inner_model.") for k in full["model"]), "the wrapper's keys, as the reference saves them"
    _run_train(b, [*common, "--end-step", "6", "--name", "run", "--resume", str(a / "run_00000003.pth")])
    resumed = torch.load(b / "run_00000006.pth", map_location="cpu", weights_only=False)
    for key in ("model", "model_ema"):
        assert full[key].keys() == resumed[key].keys()
        assert all(torch.equal(full[key][k], resumed[key][k]) for k in full[key]), key
    assert not all(torch.equal(full["model"][k], full["model_ema"][k]) for k in full["model"])
    assert full["opt"]["state"].keys() == resumed["opt"]["state"].keys() and len(full["opt"]["state"]) > 0
    for i, st in full["opt"]["state"].items():
        assert all(torch.equal(st[k], resumed["opt"]["state"][i][k]) for k in ("step", "exp_avg", "exp_avg_sq")), i
    assert full["opt"]["param_groups"] == resumed["opt"]["param_groups"]


def test_train_py_bare_greyscale_unet_on_mnist(KD, tmp_path):
    """A bare U-Net (no wrapper: no ``aug_cond`` is passed) on the resident MNIST reader, 28 -> 14 -> 7."""
    from tests.test_class_data_cpu import write_mnist
    write_mnist(tmp_path / "data")
    config = _unet_config({"type": "mnist", "location": str(tmp_path / "data")}, input_channels=1, input_size=[28, 28], depths=[1, 1, 1],
                          channels=[64, 64, 128], self_attn_depths=[False, False, True], augment_wrapper=False, augment_prob=0.0)
    (tmp_path / "config.json").write_text(json.dumps(config))
    out = _run_train(tmp_path, ["--config", str(tmp_path / "config.json"), "--batch-size", "4", "--save-every", "100", "--demo-every", "100",
                                "--seed", "1", "--end-step", "2", "--name", "run"])
    assert "Dataset resident on the device" in out.stdout
    ckpt = torch.load(tmp_path / "run_00000002.pth", map_location="cpu", weights_only=False)
    assert ckpt["step"] == 2 and not any(k.startswith("inner_model.") for k in ckpt["model"])
    assert tuple(ckpt["model"]["proj_in.weight"].shape) == (64, 1, 1, 1)


def test_train_py_unet_mixed_precision_bf16(KD, tmp_path, image_folder):
    config = _unet_config({"type": "imagefolder", "location": str(image_folder)})
    (tmp_path / "config.json").write_text(json.dumps(config))
    common = ["--config", str(tmp_path / "config.json"), "--device-augment", "--batch-size", "4", "--save-every", "100", "--demo-every", "100",
              "--seed", "1", "--num-workers", "0", "--end-step", "2", "--name", "run"]
    ckpt = {}
    for tag, extra in (("fp32", []), ("bf16", ["--mixed-precision", "bf16"])):
        (tmp_path / tag).mkdir()
        out = _run_train(tmp_path / tag, [*common, *extra])
        assert ("Mixed precision bf16" in out.stdout) == bool(extra), out.stdout[-1000:]
        if extra:
            line = next(ln for ln in out.stdout.splitlines() if "Mixed precision" in ln)
            assert line.startswith("Mixed precision bf16") and "weight-gradient convolutions and GEMMs" in line
        ckpt[tag] = torch.load(tmp_path / tag / "run_00000002.pth", map_location="cpu", weights_only=False)
    assert ckpt["fp32"]["step"] == ckpt["bf16"]["step"] == 2
    a, b = ckpt["fp32"]["model"], ckpt["bf16"]["model"]
    assert a.keys() == b.keys() and not all(torch.equal(a[k], b[k]) for k in a)

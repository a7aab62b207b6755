"""Host side of the training step, without a GPU: the LR and EMA schedules, ``ema_update_dict`` and ``make_sample_density`` against values
recorded from the reference (tests/golden/training.json, written by tests/golden/make_golden_training.py), the optimizer's state-dict
layout against ``torch.optim.AdamW``, and the refusals (there is no CPU fallback)."""
import json
import os
import types
import warnings

import pytest
import torch

from tests.golden import cases


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(cases.GOLDEN_DIR, "training.json")))


def _dummy_opt(base_lrs):
    return torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr} for lr in base_lrs], lr=1.0)


def test_lr_schedules_match_the_reference(KD, gold):
    assert {c["cls"] for c in gold["lr_sched"]} == {"InverseLR", "ExponentialLR", "ConstantLRWithWarmup"}
    assert any(c["kwargs"].get("min_lr", 0) > 0 and c["kwargs"]["warmup"] > 0 for c in gold["lr_sched"])
    for case in gold["lr_sched"]:
        cls, kw, want = getattr(KD.utils, case["cls"]), case["kwargs"], case["lrs"]
        # the closed form, on the same stand-in object the golden script called the reference's method with
        for epoch, lrs in enumerate(want):
            stand_in = types.SimpleNamespace(base_lrs=gold["base_lrs"], last_epoch=epoch, **kw)
            assert cls._get_closed_form_lr(stand_in) == lrs, (case["cls"], kw, epoch)
        # the real class, stepped over an optimizer: the same sequence bit for bit
        opt = _dummy_opt(gold["base_lrs"])
        sched = cls(opt, **kw, verbose=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for epoch, lrs in enumerate(want):
                assert sched.get_last_lr() == lrs, (case["cls"], kw, epoch)
                assert [g["lr"] for g in opt.param_groups] == lrs
                opt.step()
                sched.step()
        state = sched.state_dict()
        again = cls(_dummy_opt(gold["base_lrs"]), **kw)
        again.load_state_dict(state)
        assert again.last_epoch == sched.last_epoch and again.get_last_lr() == sched.get_last_lr()
    with pytest.raises(ValueError, match="warmup"):
        KD.utils.InverseLR(_dummy_opt([1e-3]), warmup=1.0)


def test_lr_schedules_drive_the_fused_optimizer(KD, gold):
    case = gold["lr_sched"][0]
    params = [torch.nn.Parameter(torch.zeros(2)) for _ in gold["base_lrs"]]
    opt = KD.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(params, gold["base_lrs"])])
    sched = KD.utils.InverseLR(opt, **case["kwargs"])
    for lrs in case["lrs"][:5]:
        assert [g["lr"] for g in opt.param_groups] == lrs
        opt.step()                                  # no gradients: nothing to launch
        sched.step()


def test_ema_warmup_matches_the_reference(KD, gold):
    assert any(c["kwargs"].get("start_at") and c["kwargs"].get("min_value") for c in gold["ema_warmup"])
    for case in gold["ema_warmup"]:
        sched = KD.utils.EMAWarmup(**case["kwargs"])
        values = []
        for i in range(len(case["values"])):
            values.append(sched.get_value())
            if i == 7:                              # a state_dict round trip in the middle changes nothing
                other = KD.utils.EMAWarmup()
                other.load_state_dict(sched.state_dict())
                sched = other
            sched.step()
        assert values == case["values"], case["kwargs"]
        assert sched.state_dict() == case["state_dict"]


def test_ema_update_dict_matches_the_reference(KD, gold):
    rec = gold["ema_update_dict"]
    values = {}
    for upd, decay, want in zip(rec["updates"], rec["decays"], rec["values"]):
        assert KD.utils.ema_update_dict(values, dict(upd), decay) is values
        assert values == want


def test_make_sample_density_matches_the_reference(KD, gold):
    kinds = {c["model"]["sigma_sample_density"]["type"] for c in gold["sample_density"]}
    assert kinds == {"lognormal", "loglogistic", "loguniform", "v-diffusion", "cosine", "split-lognormal", "cosine-interpolated"}
    assert sum(c["name"].endswith(".json") for c in gold["sample_density"]) >= 8
    for case in gold["sample_density"]:
        part = KD.training.make_sample_density(case["model"])
        assert part.func is getattr(KD.utils, case["func"]), case["name"]
        assert dict(part.keywords) == case["keywords"], case["name"]
        assert not part.args
    with pytest.raises(ValueError, match="Unknown sample density"):
        KD.training.make_sample_density({"sigma_data": 1.0, "sigma_sample_density": {"type": "nope"}})
    # the pinned surface of K.config stays as it is
    assert not hasattr(KD.config, "make_sample_density")


def test_optimizer_state_dict_layout_is_torch_adamw(KD):
    cfg = KD.config.load_config(cases.raw_config("tiny_sw"))
    model = KD.config.make_model(cfg)
    kw = dict(lr=3e-4, betas=(0.9, 0.95), eps=1e-6, weight_decay=1e-3)
    ours = KD.optim.AdamW(model.param_groups(3e-4), **kw)
    ref = torch.optim.AdamW(model.param_groups(3e-4), **kw)
    assert isinstance(ours, torch.optim.Optimizer)
    a, b = ours.state_dict(), ref.state_dict()
    assert a["state"] == b["state"] == {}
    assert len(a["param_groups"]) == len(b["param_groups"]) == 4
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert list(ga) == list(gb)
        assert {k: type(v) for k, v in ga.items()} == {k: type(v) for k, v in gb.items()}
        assert ga == gb
    # a torch AdamW state (the layout of a reference checkpoint's 'opt' entry) loads, key for key and dtype for dtype, and goes back
    for p in model.parameters():
        p.grad = torch.full_like(p, 1e-3)
    ref.step()
    ours.load_state_dict(ref.state_dict())
    a, b = ours.state_dict(), ref.state_dict()
    assert a["state"].keys() == b["state"].keys() and len(a["state"]) == len(list(model.parameters()))
    for i, st in b["state"].items():
        assert list(a["state"][i]) == list(st) == ["step", "exp_avg", "exp_avg_sq"]
        for k, v in st.items():
            assert a["state"][i][k].dtype == v.dtype and a["state"][i][k].shape == v.shape and torch.equal(a["state"][i][k], v), (i, k)
    torch.optim.AdamW(model.param_groups(3e-4), **kw).load_state_dict(ours.state_dict())
    with pytest.raises(ValueError, match="Invalid beta"):
        KD.optim.AdamW(model.parameters(), betas=(1.0, 0.9))


def test_training_step_has_no_cpu_fallback(KD):
    model = torch.nn.Linear(4, 4)
    avg = torch.nn.Linear(4, 4)
    opt = KD.optim.AdamW(model.parameters())
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step(clip_grad_norm=1.0)
    assert all(len(opt.state[p]) == 0 for p in model.parameters())
    with pytest.raises(RuntimeError, match="attach_ema"):
        opt.step(ema_decay=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.utils.ema_update(model, avg, 0.9)
    with pytest.raises(AssertionError):
        KD.utils.ema_update(model, torch.nn.Linear(4, 4, bias=False), 0.9)
    U = KD.utils
    for fn, kw in [(U.rand_log_normal, {}), (U.rand_log_logistic, {}), (U.rand_log_uniform, dict(min_value=0.01, max_value=80.0)),
                   (U.rand_v_diffusion, {}), (U.rand_cosine_interpolated, dict(image_d=64, noise_d_low=32, noise_d_high=64)),
                   (U.rand_split_log_normal, dict(loc=0.0, scale_1=1.0, scale_2=1.0))]:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn([4], **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.ops.sigma_density(KD._native.DENSITY_LOGUNIFORM, torch.rand(4), [0.0, 1.0])
    # the draw side is plain torch and keeps the reference's checks
    u = U.stratified_uniform([2, 8], 1, 4)
    assert torch.equal(torch.floor(u * 32).long(), (1 + torch.arange(8) * 4).expand(2, 8))
    with pytest.raises(ValueError, match="group must be"):
        U.stratified_uniform([8], 4, 4)
    with U.enable_stratified(0, 2):
        assert (U.stratified_with_settings([8]) < 0.5 + 1e-6).sum() >= 4
    assert not hasattr(U.stratified_settings, "group")
    lib = KD._native.lib()
    assert lib.kd_mt_sqnorm_f32(None, None, 0, 1.0, None, None, None) == -1 and b"kd_mt_sqnorm_f32" in lib.kd_last_error()
    assert lib.kd_mt_adamw_ema_f32(None, None, 0, None, 0, None, 0.0, 0, 0, None) == -1
    assert lib.kd_mt_lerp_f32(None, None, 0, 0.5, None) == -1
    assert lib.kd_sigma_density_f32(9, None, 0, None, None, 0, 4, 4, 0, 0, None, None) == -1


def test_image_folder_and_csv_logger(KD, tmp_path):
    from PIL import Image
    (tmp_path / "sub").mkdir()
    Image.new("RGB", (40, 20), (255, 0, 0)).save(tmp_path / "b.png")
    Image.new("L", (10, 30), 128).save(tmp_path / "sub" / "a.png")
    (tmp_path / "notes.txt").write_text("x")
    ds = KD.utils.FolderOfImages(tmp_path, transform=lambda im: KD.utils.from_pil_image(KD.utils.resize_center_crop(im, 16)))
    assert len(ds) == 2 and [p.name for p in ds.paths] == ["b.png", "a.png"]
    (x,), (y,) = ds[0], ds[1]
    assert x.shape == y.shape == (3, 16, 16) and x.dtype == torch.float32
    assert torch.equal(x[0], torch.ones(16, 16)) and torch.equal(x[1], -torch.ones(16, 16))
    assert (y - (128 / 255 * 2 - 1)).abs().max() < 1e-6
    assert KD.utils.FolderOfImages(tmp_path)[0][0].size == (40, 20)
    log = KD.utils.CSVLogger(tmp_path / "log.csv", ["step", "loss"])
    log.write(0, 0.5)
    KD.utils.CSVLogger(tmp_path / "log.csv", ["step", "loss"]).write(1, 0.25)
    assert (tmp_path / "log.csv").read_text() == "step,loss\n0,0.5\n1,0.25\n"


def test_train_py_refuses_what_it_does_not_implement(KD, tmp_path):
    import subprocess
    import sys
    train = os.path.join(cases.REPO, "train.py")
    env = dict(os.environ, PYTHONPATH=cases.REPO)
    for flags, msg in [(["--gns"], "gns"), (["--wandb-project", "x"], "wandb"), (["--evaluate-every", "10"], "evaluation")]:
        out = subprocess.run([sys.executable, train, "--config", "none.json", *flags], capture_output=True, text=True, env=env)
        assert out.returncode == 2 and msg in out.stderr, out.stderr
    raw = cases.raw_config("tiny_global")
    for patch, msg in [({"model": {"augment_prob": 0.12}}, "augment_prob"), ({"optimizer": {"type": "sgd"}}, "adamw"),
                       ({"dataset": {"type": "cifar10", "location": "x"}}, "imagefolder")]:
        cfg = json.loads(json.dumps(raw))
        cfg.setdefault("dataset", {"type": "imagefolder", "location": str(tmp_path)})
        for k, v in patch.items():
            cfg.setdefault(k, {}).update(v)
        path = tmp_path / "cfg.json"
        path.write_text(json.dumps(cfg))
        out = subprocess.run([sys.executable, train, "--config", str(path)], capture_output=True, text=True, env=env)
        assert out.returncode != 0 and "NotImplementedError" in out.stderr and msg in out.stderr, out.stderr[-500:]

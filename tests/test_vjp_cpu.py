"""Host side of the input-gradient route (no GPU): when a model call becomes an autograd node, what it refuses before any kernel runs,
and the per-model cache of transposed weights behind the backward pass."""
import importlib

import pytest
import torch

from tests.golden import cases


def _model(KD, name="tiny_global"):
    cfg = KD.config.load_config(cases.raw_config(name))
    model = KD.config.make_model(cfg).eval().requires_grad_(False)
    model.load_state_dict(KD.synth.synth_state_dict(model.state_dict(), seed=cases.WEIGHT_SEED))
    return cfg, model


def test_conditioning_gradients_are_refused(KD):
    cfg, model = _model(KD, "tiny_sw")
    den = KD.Denoiser(model, 0.5)
    x = torch.randn(1, 3, 32, 32, requires_grad=True)
    cls = torch.tensor([1])
    with torch.enable_grad():
        with pytest.raises(NotImplementedError, match="w.r.t. sigma"):
            den(x, torch.ones(1, requires_grad=True), class_cond=cls)
        with pytest.raises(NotImplementedError, match="w.r.t. aug_cond"):
            model(x, torch.ones(1), aug_cond=torch.zeros(1, 9, requires_grad=True), class_cond=cls)
        with pytest.raises(NotImplementedError, match="w.r.t. mapping_cond"):
            model(x, torch.ones(1), class_cond=cls, mapping_cond=torch.zeros(1, 4, requires_grad=True))
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # the grad route fails as forward does
            den(x, torch.ones(1), class_cond=cls)


def test_no_grad_calls_stay_on_the_plain_path(KD, monkeypatch):
    """Without grad mode, or with an x that does not require grad, the call never becomes an autograd node."""
    cfg, model = _model(KD)
    itv2 = importlib.import_module(KD.__name__ + ".models.image_transformer_v2")
    calls = []
    monkeypatch.setattr(itv2._InputGrad, "apply", lambda *a: calls.append(a))
    x = torch.randn(1, 3, 16, 16)
    for ctx, req in ((torch.no_grad(), True), (torch.enable_grad(), False)):
        with ctx:
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                model(x.clone().requires_grad_(req), torch.ones(1))
    assert not calls
    with torch.enable_grad():
        model(x.clone().requires_grad_(), torch.ones(1))
    assert len(calls) == 1


def test_transposed_weights_are_cached_per_model(KD):
    cfg, model = _model(KD)
    vjp = importlib.import_module(KD.__name__ + ".models.vjp")
    w = model.patch_in.proj.weight
    t = vjp._wt(model, w)
    assert torch.equal(t, w.t()) and t.is_contiguous()
    assert vjp._wt(model, w) is t                                        # built once
    with torch.no_grad():
        w.mul_(2.0)                                                      # an in-place update builds it again
    t2 = vjp._wt(model, w)
    assert t2 is not t and torch.equal(t2, w.t())
    cfg, model = _model(KD, "tiny_sw")
    sp = model.splits[0]
    tf = vjp._wt(model, sp.proj.weight, fac=sp.fac)
    assert torch.allclose(tf, (sp.proj.weight * sp.fac).t())
    with torch.no_grad():
        sp.fac.fill_(0.25)
    assert torch.allclose(vjp._wt(model, sp.proj.weight, fac=sp.fac), (sp.proj.weight * 0.25).t())


def test_invalidate_drops_the_derived_tensors(KD):
    """A weight made under torch.inference_mode() has no version counter, so an in-place edit of it leaves no trace: invalidate() is the
    way to say so, and it drops what the backward and dual passes derived from the weights, as it drops the plans."""
    cfg, model = _model(KD)
    vjp = importlib.import_module(KD.__name__ + ".models.vjp")
    with torch.inference_mode():
        w = torch.randn(8, 4)
    t = vjp._wt(model, w)
    assert torch.equal(t, w.t()) and vjp._wt(model, w) is t
    with torch.inference_mode():
        w.mul_(2.0)
    model.invalidate()
    assert torch.equal(vjp._wt(model, w), w.t())

"""k_diffusion_amd.weights without a GPU: tensor identity, the weak per-tensor cache, the weights fingerprint of both model families (the
HDiT walk is tests/test_host_cpu.py::test_weights_fingerprint_keeps_its_tensor_list_and_still_sees_every_change) and the plan cache."""
import copy
import gc
import os
import weakref

import pytest
import torch
from torch import nn

import k_diffusion_amd as K
from k_diffusion_amd import weights
from tests import unet_ref as ur

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unet():
    model = K.config.make_model(K.config.load_config(ur.CONFIGS["unet_a"])).eval().requires_grad_(False)
    return getattr(model, "inner_model", model)


def hdit():
    return K.config.make_model(K.config.load_config(os.path.join(REPO, "configs", "config_mnist_transformer.json"))).eval().requires_grad_(False)


def test_ident_is_address_version_shape():
    t = torch.zeros(3, 4)
    assert weights.ident(None) is None and weights.ident(t) == (t.data_ptr(), t._version, (3, 4)) == weights.ident(t)
    before = weights.ident(t)
    t.add_(1.0)
    assert weights.ident(t) != before and weights.ident(t[1]) != weights.ident(t)
    with torch.inference_mode():
        i = torch.zeros(3)
    assert weights.ident(i) != weights.ident(i) and weights.version(i) != weights.version(i)
    assert weights.ident(i, never_same=False) == weights.ident(i, never_same=False) == (i.data_ptr(), None, (3,))


# ---- the weak cache -------------------------------------------------------------------------------------------------------------------------

def counting():
    built = []

    def build():
        built.append(object())
        return built[-1]
    return built, build


def test_weak_cache_hits_and_misses():
    cache, (built, build) = weights.WeakCache(), counting()
    w = torch.zeros(4, 4)
    v = cache.get(w, "a", (4, 4), build)
    assert cache.get(w, "a", (4, 4), build) is v and len(built) == 1                        # hit
    assert cache.get(w, "b", (4, 4), build) is not v and len(built) == 2                    # another extra key: an entry of its own
    assert cache.get(w, "a", (4, 4), build) is v and cache.get(w, "a", (2, 8), build) is not v and len(built) == 3       # the caller's meta moved
    w.mul_(2.0)
    v2 = cache.get(w, "a", (2, 8), build)
    assert v2 is not built[2] and len(built) == 4                                             # an in-place edit
    assert cache.get(w, "a", (2, 8), build, cache=False) is not v2 and cache.get(w, "a", (2, 8), build) is v2 and len(built) == 5
    # a new tensor at a recycled id: the old entry (kept by hand, as if its weakref callback had not run yet) must not serve it
    old_key, old_ent = next((k, e) for k, e in cache.entries.items() if k[1] == "b")
    other = torch.ones(4, 4)
    cache.entries[(id(other), "b")] = old_ent
    assert cache.get(other, "b", (4, 4), build) is built[5] and len(built) == 6
    # inference-mode tensors: never cached
    with torch.inference_mode():
        i = torch.zeros(4, 4)
    n = len(cache.entries)
    assert cache.get(i, "a", (4, 4), build) is not cache.get(i, "a", (4, 4), build) and len(cache.entries) == n and len(built) == 8
    # the entry dies with the tensor
    assert any(k[0] == id(w) for k in cache.entries)
    wid = id(w)
    del w
    gc.collect()
    assert not any(k[0] == wid for k in cache.entries)


class AllocatingKey:
    """An ``extra`` key whose hash allocates a container and keeps it: whatever hashes cache keys in a loop feeds the cycle collector's counter."""

    def __init__(self):
        self.kept = []

    def __hash__(self):
        self.kept.append([])
        return 7


@pytest.mark.parametrize("after", range(1, 9))
def test_weak_cache_prune_survives_a_collection_in_its_middle(after):
    """Past the bound the cache prunes; the tensors of most entries are unreachable by then but sit in reference cycles, so only the cycle
    collector frees them -- and it runs INSIDE the prune, where every freed tensor's weakref callback deletes from the cache's dict: the
    ``build`` of the call that prunes switches the collector on, due ``after`` container allocations later."""
    cache, (built, build), extra = weights.WeakCache(), counting(), AllocatingKey()
    live = [torch.zeros(2) for _ in range(5)]
    values = [cache.get(t, extra, None, build) for t in live]
    old = gc.get_threshold()
    gc.collect()
    gc.disable()
    try:
        for _ in range(cache.bound + 1 - len(live)):          # one more entry than the bound: the next insertion prunes
            t = torch.zeros(1)
            t.cycle = t                           # unreachable after this iteration, freed only by the collector
            cache.get(t, extra, None, build)
        del t
        assert len(cache.entries) == cache.bound + 1

        def build_and_arm():
            gc.set_threshold(gc.get_count()[0] + after, 10, 10)
            gc.enable()
            return "new"
        new = torch.zeros(3)
        assert cache.get(new, extra, None, build_and_arm) == "new"
    finally:
        gc.set_threshold(*old)
        gc.enable()
    n = len(built)
    assert [cache.get(t, extra, None, build) for t in live] == values and len(built) == n    # the live entries survived
    assert cache.get(new, extra, None, build) == "new" and len(cache.entries) == len(live) + 1


# ---- WeightWatch ----------------------------------------------------------------------------------------------------------------------------

def test_watch_sees_every_change_of_the_unet_without_walking_it():
    m = unet()
    f = [m._weights_fingerprint()]
    assert len(f[0]) == 1 + len(list(m.parameters())) + len(list(m.buffers()))
    walked, orig = [], nn.Module.modules

    def moved(walks):
        f.append(m._weights_fingerprint())
        assert f[-1] != f[-2] and bool(walked) == walks, (len(f), walked)
        del walked[:]
    try:
        nn.Module.modules = lambda self, *a, **k: (walked.append(1), orig(self, *a, **k))[1]
        assert m._weights_fingerprint() == f[0] and not walked                          # unchanged: the kept list, no traversal
        m.load_state_dict(K.synth.synth_state_dict(m.state_dict(), seed=1))
        moved(False)
        conv = m.u_net.d_blocks[0][1].main[2]
        with torch.no_grad():
            conv.weight.mul_(2.0)                                                       # in place
        moved(False)
        conv.weight = nn.Parameter(torch.zeros_like(conv.weight), requires_grad=False)  # a parameter assigned anew
        moved(True)
        assert any(t is conv.weight for t in m._watch.tensors)
        conv.bias.data = conv.bias.data.clone()                                         # .data swapped: same Parameter, other storage
        moved(False)
        m.proj_out._parameters["weight"] = nn.Parameter(m.proj_out.weight.detach().clone() + 1.0, requires_grad=False)      # past __setattr__
        moved(True)
        assert any(t is m.proj_out._parameters["weight"] for t in m._watch.tensors)
        m.proj_in = nn.Conv2d(m.proj_in.in_channels, m.proj_in.out_channels, 1).requires_grad_(False)                        # a sub-module replaced
        moved(True)
        m.invalidate()
        moved(False)
        m.double()
        f.append(m._weights_fingerprint())
        assert f[-1] != f[-2]
    finally:
        nn.Module.modules = orig


@pytest.mark.parametrize("make", [unet, hdit])
def test_watch_sees_inference_mode_weights_reloaded(make):
    """Weights made under torch.inference_mode() carry no version counter: the load_state_dict post-hooks (of the root and of any
    sub-module) and invalidate() move the fingerprint."""
    with torch.inference_mode():
        m = make()
        f0 = m._weights_fingerprint()
        m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
        f1 = m._weights_fingerprint()
        assert f1 != f0 and [e[1:] for e in f1[1:]] == [e[1:] for e in f0[1:]]           # (nothing but the epoch can tell)
        sub = next(c for c in m.modules() if c is not m and list(c.parameters(recurse=False)))
        sub.load_state_dict(sub.state_dict())
        f2 = m._weights_fingerprint()
        assert f2 != f1
    m.invalidate()
    assert m._weights_fingerprint() != f2


@pytest.mark.parametrize("make", [unet, hdit])
def test_a_deep_copy_watches_its_own_tree(make):
    m = make()
    m._weights_fingerprint()                      # the original's hooks are installed before the copy is made, as in train.py
    c = copy.deepcopy(m)
    assert c._watch is not m._watch and c._watch.root() is c and c._plans is c._plan_cache.plans is not m._plans
    fm, fc = m._weights_fingerprint(), c._weights_fingerprint()
    assert all(any(t is p for p in c.parameters()) or any(t is b for b in c.buffers()) for t in c._watch.tensors)
    c.load_state_dict(c.state_dict())
    assert c._watch.epoch > fc[0] and c._weights_fingerprint() != fc and m._weights_fingerprint() == fm
    fc = c._weights_fingerprint()
    m.load_state_dict(m.state_dict())
    assert m._watch.epoch > fm[0] and m._weights_fingerprint() != fm and c._weights_fingerprint() == fc
    fm = m._weights_fingerprint()
    c.invalidate()
    assert c._weights_fingerprint() != fc and m._weights_fingerprint() == fm
    fc = c._weights_fingerprint()
    m.invalidate()
    assert m._weights_fingerprint() != fm and c._weights_fingerprint() == fc
    # a copy of a copy, and a second fingerprint of the same tree, install no second hook
    c2 = copy.deepcopy(c)
    c2._weights_fingerprint()
    assert all(len(mod._load_state_dict_post_hooks) == 1 for mod in c2.modules())
    # the hooks do not keep a model alive
    refs = [weakref.ref(x) for x in (m, c, c2)]
    del m, c, c2
    gc.collect()
    assert all(r() is None for r in refs)


# ---- PlanCache ------------------------------------------------------------------------------------------------------------------------------

class FakePlan:
    def __init__(self, name, device, log):
        self.name, self.device, self.log = name, device, log

    def release(self):
        self.log.append(("release", self.name))


def test_plan_cache_is_least_recently_used_with_the_bound_of_each_call():
    log = []
    cache = weights.PlanCache(synchronize=lambda device: log.append(("sync", device)))
    for name in "abcd":
        assert cache.put(name, lambda: FakePlan(name, "gpu0" if name < "c" else "gpu1", log), 4).name == name
    assert list(cache.plans) == list("abcd") and not log
    assert cache.get("a").name == "a" and cache.get("x") is None and list(cache.plans) == list("bcda")       # a: most recently used now
    cache.put("e", lambda: FakePlan("e", "gpu1", log), 4)
    assert list(cache.plans) == list("cdae")
    # the evicted plan's OWN device was synchronised (b: gpu0, the newcomer lives on gpu1), before its release
    assert log == [("sync", "gpu0"), ("release", "b")]
    del log[:]
    cache.put("f", lambda: FakePlan("f", "gpu0", log), 2)                                                    # the bound changed between calls
    assert list(cache.plans) == list("ef") and log == [("sync", "gpu1"), ("sync", "gpu0"), ("release", "c"), ("release", "d"), ("release", "a")]
    del log[:]
    cache.put("g", lambda: FakePlan("g", "gpu1", log), 8)
    assert list(cache.plans) == list("efg") and not log
    # the dict is the plain dict callers read
    assert dict(cache.plans).keys() == cache.plans.keys() and len(cache.plans) == 3 and cache.plans["f"].name == "f"
    cache.drop_all()
    assert not cache.plans and sorted(log[:2]) == [("sync", "gpu0"), ("sync", "gpu1")] and log[2:] == [("release", n) for n in "efg"]
    del log[:]
    cache.drop_all()
    assert not log
    # a plan without release() (the U-Net's) is accepted: nothing to give back, nothing to wait for
    cache.put(1, lambda: object(), 2), cache.put(2, lambda: object(), 2), cache.put(3, lambda: object(), 2)
    assert list(cache.plans) == [2, 3] and not log
    cache.drop_all()
    assert not cache.plans and not log


def test_plan_cache_default_synchronize_ignores_other_devices():
    log = []
    cache = weights.PlanCache()
    cache.put("a", lambda: FakePlan("a", torch.device("cpu"), log), 1)
    cache.put("b", lambda: FakePlan("b", None, log), 1)
    cache.drop_all()
    assert log == [("release", "a"), ("release", "b")]

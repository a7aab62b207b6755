"""Host-side bookkeeping that tells whether a cached value still belongs to the tensors it was made from -- one definition of each idea, for
every model family (plain Python and torch: no kernel, no library):

* ``version`` / ``ident``: 'the same tensor data as last time';
* ``WeakCache``: a value per tensor OBJECT (packed weight images), which dies with the tensor;
* ``WeightWatch``: the fingerprint of all weights of one model, read on every model call;
* ``PlanCache``: a model's launch plans, least recently used first out.
"""
import copy
import gc
from functools import partial
import itertools
import operator
import weakref

import torch

_untracked = itertools.count(-1, -1)


def version(t, never_same=True):
    """Version counter of a tensor, or a value that never repeats for tensors made under torch.inference_mode() (they carry no
    counter, so an in-place change cannot be seen: such a tensor is never recognised as 'the same data as last time').  With
    ``never_same=False`` those give None instead: for a store that is told of such edits another way (``invalidate()``)."""
    if not t.is_inference():
        return t._version
    return next(_untracked) if never_same else None


def ident(t, never_same=True):
    """(address, version, shape) of a tensor; None passes through.  Whoever compares two of these must keep the first tensor alive
    in between, or its address may have been handed to another tensor."""
    return None if t is None else (t.data_ptr(), version(t, never_same), tuple(t.shape))


class WeakCache:
    """``build()`` results per tensor object and ``extra`` key (packed images of weights, which are static while sampling).  An entry is
    valid while the weak reference is alive and ``ident(t)`` and the caller's ``meta`` are what they were, so a new tensor that happens
    to reuse the id or the address of a freed one never hits a stale value; it goes when the tensor dies (plans pack per-plan
    concatenations of weights).  Tensors made under torch.inference_mode() have no version counter to tell a rewritten tensor by: never
    cached.  Beyond ``bound`` entries the dead ones are pruned, then everything is dropped."""

    def __init__(self, bound=512):
        self.bound, self.entries = bound, {}

    def _gone(self, key, ref):
        ent = self.entries.get(key)
        if ent is not None and ent[0] is ref:
            del self.entries[key]

    def get(self, t, extra, meta, build, cache=True):
        if not cache or t.is_inference():
            return build()
        key = (id(t), extra)
        ent = self.entries.get(key)
        if ent is not None and ent[0]() is t and ent[1] == (ident(t), meta):
            return ent[2]
        value = build()
        if len(self.entries) > self.bound:
            # a garbage collection during the loop runs ``_gone`` for every tensor it frees, which deletes from ``self.entries``: the dict
            # that is walked is set aside first, so nothing writes to it (``dict.copy()`` itself may collect between reading and counting)
            old, self.entries = self.entries, {}
            for k, e in old.items():
                if e[0]() is not None:
                    self.entries[k] = e
            if len(self.entries) > self.bound:
                self.entries.clear()
        self.entries[key] = (weakref.ref(t, partial(self._gone, key)), (ident(t), meta), value)
        return value


class _Bump:
    """load_state_dict post-hook that bumps a watch's epoch.  It holds the watch weakly (a sub-module shared with another model does not
    pin this one), and its deep copy belongs to the watch's copy: ``copy.deepcopy(model)`` copies the hook dicts of every module."""

    def __init__(self, watch):
        self.watch = weakref.ref(watch)

    def __call__(self, *_args):
        watch = self.watch()
        if watch is not None:
            watch.bump()

    def __deepcopy__(self, memo):
        watch = self.watch()
        return self if watch is None else _Bump(copy.deepcopy(watch, memo))


class WeightWatch:
    """The weights fingerprint of the module tree under ``root``; one per model, which holds the only strong reference to it.

    ``fingerprint()``: (address, version) of every parameter and buffer (behind a per-model epoch): a changed entry drops the plans and
    the packed weight images.  Read on every model call, so the LIST of tensors is kept (``tensors``) -- torch's module traversal
    (parameters() / buffers() over ~90 sub-modules) took 0.3 - 0.4 ms per call, more than the launches of a batch-1 forward.  What makes
    the kept list safe is a per-call identity check of every SLOT the tree has -- each (module._parameters | _buffers | _modules dict,
    name) still holds the object it held when the list was built, and each of those dicts still has the size it had (a parameter /
    buffer / sub-module ADDED to an existing module) -- which is ~300 dict reads in C (a few microseconds), needs no traversal and sees
    the ways a tensor can be swapped: attribute assignment, register_*, del + re-register, a replaced sub-module, and direct writes into
    ``module._parameters[name]`` (torch.func.functional_call / stateless._reparametrize_module swap parameters that way, past every
    registration hook).  In-place edits move the tensors' version counters; .to() moves their addresses; ``bump()`` -- called by the
    load_state_dict post-hooks this installs on every module of the tree, and by the model's ``_apply`` and ``invalidate()`` -- moves
    the epoch (which also covers inference-mode tensors, whose edits leave no version trace).  No process-wide hooks: only this model's
    own tree is looked at.

    A deep copy of a model gets a fresh watch of the COPIED tree, and the copied modules' hooks bump that one (``_Bump``)."""

    def __init__(self, root):
        self.root, self.epoch = weakref.ref(root), 0
        self.tensors, self._tracked = (), ()
        self._dicts, self._names, self._objs, self._sized, self._sizes = (), (), (), (), ()

    def __deepcopy__(self, memo):
        root = memo.get(id(self.root()))
        return self if root is None else WeightWatch(root)      # (a sub-module copied on its own stays with this watch)

    def bump(self):
        self.epoch += 1

    def fingerprint(self):
        if not (self._objs and all(map(operator.is_, map(dict.get, self._dicts, self._names), self._objs))
                and tuple(map(len, self._sized)) == self._sizes):      # (sizes: a slot ADDED to a recorded dict is no recorded slot)
            self._walk()
        return (self.epoch, *[(t.data_ptr(), t._version if tr else 0) for t, tr in zip(self.tensors, self._tracked)])

    def _walk(self):
        dicts, names, objs, ts, sized = [], [], [], [], []
        for mod in self.root().modules():
            # a (sub-)module's load_state_dict rewrites weights in place: bump the epoch (inference-mode tensors)
            if not any(isinstance(h, _Bump) and h.watch() is self for h in mod._load_state_dict_post_hooks.values()):
                mod.register_load_state_dict_post_hook(_Bump(self))
            for d, is_tensor in ((mod._parameters, True), (mod._buffers, True), (mod._modules, False)):
                sized.append(d)
                for name, obj in d.items():
                    dicts.append(d), names.append(name), objs.append(obj)
                    if is_tensor and obj is not None:
                        ts.append(obj)
        uniq = list({id(t): t for t in ts}.values())                  # tied tensors once, like parameters() / buffers()
        self._dicts, self._names, self._objs = tuple(dicts), tuple(names), tuple(objs)
        self._sized, self._sizes = tuple(sized), tuple(map(len, sized))
        self.tensors, self._tracked = tuple(uniq), tuple(not t.is_inference() for t in uniq)


def _synchronize(device):
    if getattr(device, "type", "cpu") == "cuda":
        torch.cuda.synchronize(device)


class PlanCache:
    """A model's launch plans by key, least recently used first out: ``plans`` is the plain dict, most recently used last (dicts keep
    insertion order).  A plan that goes gives its workspaces back at once through its ``release()``, if it has one; its own ``device`` is
    idle first (``synchronize``): the plan's side-stream work may still be reading buffers the allocator would hand out again.  One
    run of the cycle collector follows a drop, for the plans' helper objects' own cycles."""

    def __init__(self, synchronize=_synchronize):
        self.plans, self.synchronize = {}, synchronize

    def get(self, key):
        plan = self.plans.get(key)
        if plan is not None and len(self.plans) > 1:
            self.plans[key] = self.plans.pop(key)
        return plan

    def put(self, key, build, bound):
        """Make room for one more within ``bound`` (read by the caller at call time), then keep ``build()`` under ``key``."""
        self._drop(list(self.plans)[:max(0, len(self.plans) - bound + 1)])
        plan = self.plans[key] = build()
        return plan

    def drop_all(self):
        self._drop(list(self.plans))

    def _drop(self, keys):
        if not keys:
            return
        held = [p for p in map(self.plans.pop, keys) if hasattr(p, "release")]
        for device in dict.fromkeys(p.device for p in held):         # each distinct device once
            self.synchronize(device)
        for p in held:
            p.release()
        gc.collect()

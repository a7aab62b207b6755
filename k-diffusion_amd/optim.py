"""The optimizer step of the reference's training loop (train.py:463-473) on the multi-tensor HIP kernels of csrc/optim_f32.hip:
``clip_grad_norm_`` + ``torch.optim.AdamW.step`` + ``K.utils.ema_update`` + ``zero_grad(set_to_none=False)`` as one norm launch (two
kernels) and one fused launch over every parameter, instead of a few foreach passes and one ``lerp_`` launch per parameter.

``AdamW`` is a ``torch.optim.Optimizer``: LR schedulers, ``param_groups`` and ``state_dict()`` / ``load_state_dict()`` are torch's (the
state has torch AdamW's layout, so checkpoints interchange with ``torch.optim.AdamW`` in both directions).  Parameters must be fp32,
contiguous and on a ROCm device -- anything else raises (there is no eager fallback).
"""
import ctypes as C
import weakref

import torch

from . import _native as nat
from .ops import _chk, _stream


class MultiTensorTable:
    """The device-resident descriptor table of a multi-tensor launch (include/kdiff_hip.h: KdMtTensor + the chunk list).  ``update`` takes one
    tuple (p, g, m, v, ema, n, group) of addresses / sizes per tensor and refreshes the device copy only when a tuple changed: an asynchronous
    copy from freshly pinned host memory on the current stream (no synchronisation; the stream orders it against the launches that read it)."""

    def __init__(self):
        self.key = None
        self.table = self.chunks = None
        self.n_chunks = 0

    def update(self, entries, device):
        key = (tuple(entries), str(device))
        if key == self.key:
            return
        arr = (nat.KdMtTensor * len(entries))()
        chunks = []
        for i, (p, g, m, v, ema, n, group) in enumerate(entries):
            e = arr[i]
            e.p, e.g, e.m, e.v, e.ema, e.n, e.group = p, g, m, v, ema, n, group
            chunks += [(i, c) for c in range((n + nat.MT_CHUNK - 1) // nat.MT_CHUNK)]
        host = torch.empty(C.sizeof(arr), dtype=torch.uint8, pin_memory=True)
        C.memmove(host.data_ptr(), C.addressof(arr), C.sizeof(arr))
        host_chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1).pin_memory()
        if self.table is None or self.table.numel() != host.numel() or self.table.device != device:
            self.table = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        if self.chunks is None or self.chunks.numel() != host_chunks.numel() or self.chunks.device != device:
            self.chunks = torch.empty(host_chunks.numel(), dtype=torch.int32, device=device)
        self.table.copy_(host, non_blocking=True)
        self.chunks.copy_(host_chunks, non_blocking=True)
        self.n_chunks = len(chunks)
        self.key = key

    def args(self):
        return C.c_void_p(self.table.data_ptr()), C.c_void_p(self.chunks.data_ptr()), self.n_chunks


def _ptr(t):
    return t.data_ptr()


def lerp_(pairs, weight, table):
    """``avg.lerp_(p, weight)`` for every (p, avg) pair in one kd_mt_lerp_f32 launch; bumps the version counters of the written tensors."""
    if not pairs:
        return
    for i, (p, avg) in enumerate(pairs):
        _chk(p, f"ema_update: parameter {i}")
        _chk(avg, f"ema_update: averaged parameter {i}")
        if p.shape != avg.shape or p.device != avg.device:
            raise ValueError(f"ema_update: parameter {i}: {tuple(p.shape)} on {p.device} against {tuple(avg.shape)} on {avg.device}")
    table.update([(_ptr(p), 0, 0, 0, _ptr(avg), p.numel(), 0) for p, avg in pairs if p.numel()], pairs[0][0].device)
    if table.n_chunks:
        nat.check(nat.lib().kd_mt_lerp_f32(*table.args(), float(weight), _stream()), "kd_mt_lerp_f32")
        torch.autograd.graph.increment_version([avg for _, avg in pairs])


def paired(model, averaged_model):
    """(parameter pairs, buffer pairs) of a model and its averaged copy, by name; equal key sets asserted (utils.py:92-101)."""
    params, avg_params = dict(model.named_parameters()), dict(averaged_model.named_parameters())
    assert params.keys() == avg_params.keys()
    bufs, avg_bufs = dict(model.named_buffers()), dict(averaged_model.named_buffers())
    assert bufs.keys() == avg_bufs.keys()
    return [(p, avg_params[n]) for n, p in params.items()], [(b, avg_bufs[n]) for n, b in bufs.items()]


class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` (amsgrad=False, maximize=False) on the fused HIP step.

    ``step(clip_grad_norm=None, ema_decay=None, zero_grad=False)`` runs, without a host synchronisation,
      * with ``clip_grad_norm``: the global gradient norm (kd_mt_sqnorm_f32) -- returned as a 0-d device tensor -- and
        ``clip_grad_norm_``'s coefficient, applied to the gradients as the update reads them (the stored gradients stay unclipped);
      * AdamW's update of every parameter that has a gradient;
      * with ``ema_decay`` and a model attached by ``attach_ema``: ``K.utils.ema_update(model, averaged_model, ema_decay)``;
      * with ``zero_grad``: ``zero_grad(set_to_none=False)``, in the same pass (the gradient buffers and their addresses stay).
    The parameters are written through raw pointers, so the step bumps their version counters itself: the model's launch plan and packed
    weight images are keyed on them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr must be a float: the fused step takes its constants by value")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # torch.optim.AdamW's group keys, so that state dicts interchange; the switches keep the values this step implements
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._table = MultiTensorTable()
        self._rest_table = MultiTensorTable()
        self._ema = {}                 # parameter -> its averaged copy
        self._ema_pairs = []
        self._ema_buffers = []

    def attach_ema(self, model, averaged_model):
        """Pair ``model``'s parameters with ``averaged_model``'s by name for ``step(ema_decay=...)``; buffers are copied on such a step."""
        pairs, self._ema_buffers = paired(model, averaged_model)
        self._ema_pairs = pairs
        self._ema = {p: avg for p, avg in pairs}

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
            raise NotImplementedError("the fused AdamW step implements amsgrad=False, maximize=False, capturable=False, differentiable=False")
        if not group.get("decoupled_weight_decay", True):
            raise NotImplementedError("the fused AdamW step implements the decoupled weight decay only")
        if isinstance(group["lr"], torch.Tensor):
            raise NotImplementedError("a tensor lr is not supported: the fused step takes its constants by value")

    @torch.no_grad()
    def step(self, clip_grad_norm=None, ema_decay=None, zero_grad=False):
        use_ema = ema_decay is not None
        if use_ema and not self._ema_pairs:
            raise RuntimeError("step(ema_decay=...) needs attach_ema(model, averaged_model) first")
        entries, buckets, written, grads, steps, device = [], {}, [], [], [], None
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                _chk(p, "AdamW.step: parameter")
                _chk(g, "AdamW.step: gradient")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError(f"AdamW.step: parameters on {device} and {p.device}; one optimizer steps one device")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = _chk(state["exp_avg"], "AdamW.step: exp_avg"), _chk(state["exp_avg_sq"], "AdamW.step: exp_avg_sq")
                if m.shape != p.shape or v.shape != p.shape or g.shape != p.shape:
                    raise ValueError("AdamW.step: gradient / state shape differs from the parameter's")
                step_t = state["step"]
                steps.append(step_t)
                # parameters of a group that have taken different numbers of steps (a gradient was None on some) get a bucket each:
                # the bias corrections are per step count
                bucket = buckets.setdefault((gi, float(step_t) + 1.0), len(buckets))
                avg = self._ema.get(p) if use_ema else None
                if avg is not None:
                    _chk(avg, "AdamW.step: averaged parameter")
                if p.numel():
                    entries.append((_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(avg) if avg is not None else 0, p.numel(), bucket))
                written.append(p)
                grads.append(g)
        norm = None
        if entries:
            lib = nat.lib()
            self._table.update(entries, device)
            clip = None
            if clip_grad_norm is not None:
                ws = torch.empty(self._table.n_chunks, dtype=torch.float64, device=device)
                pair = torch.empty(2, dtype=torch.float32, device=device)
                nat.check(lib.kd_mt_sqnorm_f32(*self._table.args(), float(clip_grad_norm), C.c_void_p(ws.data_ptr()),
                                               C.c_void_p(pair.data_ptr()), _stream()), "kd_mt_sqnorm_f32")
                clip, norm = C.c_void_p(pair.data_ptr()), pair[0]
            torch._foreach_add_(steps, 1)
            consts = (nat.KdAdamGroup * len(buckets))()
            for (gi, step), b in buckets.items():
                group, c = self.param_groups[gi], consts[b]
                beta1, beta2 = group["betas"]
                c.lr, c.wd, c.beta1, c.beta2, c.eps = float(group["lr"]), float(group["weight_decay"]), float(beta1), float(beta2), float(group["eps"])
                c.bc1, c.bc2 = 1 - beta1 ** step, 1 - beta2 ** step
            nat.check(lib.kd_mt_adamw_ema_f32(*self._table.args(), consts, len(buckets), clip, float(ema_decay) if use_ema else 0.0,
                                              1 if use_ema else 0, 1 if zero_grad else 0, _stream()), "kd_mt_adamw_ema_f32")
            torch.autograd.graph.increment_version(written)
            if zero_grad:
                torch.autograd.graph.increment_version(grads)
        elif clip_grad_norm is not None:
            raise RuntimeError("AdamW.step(clip_grad_norm=...): no parameter has a gradient")
        if use_ema:
            done = set(written)
            torch.autograd.graph.increment_version([self._ema[p] for p in written if p in self._ema])
            # parameters this step did not update (no gradient, or not this optimizer's) still enter the average, as in K.utils.ema_update
            lerp_([(p, avg) for p, avg in self._ema_pairs if p not in done], 1 - ema_decay, self._rest_table)
            for buf, avg in self._ema_buffers:
                avg.copy_(buf)
        return norm


_ema_tables = weakref.WeakKeyDictionary()      # averaged model -> its stand-alone lerp table


def ema_update(model, averaged_model, decay):
    """K.utils.ema_update (utils.py:88-104): one kd_mt_lerp_f32 launch over all parameters, then the buffer copies."""
    with torch.no_grad():
        pairs, buffers = paired(model, averaged_model)
        table = _ema_tables.get(averaged_model)
        if table is None:
            table = _ema_tables[averaged_model] = MultiTensorTable()
        lerp_(pairs, 1 - decay, table)
        for buf, avg in buffers:
            avg.copy_(buf)

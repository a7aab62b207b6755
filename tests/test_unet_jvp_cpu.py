"""The dual (forward-mode JVP) pass of the image_v1 U-Net without a GPU: the ABI of its three entry points, the refusals that need no device,
and the differentiable restatement that tests/test_unet_jvp_gpu.py takes its tangents from (it must be ``unet_ref.forward`` exactly)."""
import ctypes as C
import math
import os
import re

import pytest
import torch
from torch.nn import functional as F

from tests import unet_ref as ur
from tests.test_unet_cpu import built

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = {"kd_conv2d_x3_stacked": 16, "kd_groupnorm_stats_jvp_f32": 12, "kd_adagn_apply_jvp_f32": 18}
F64 = torch.float64


# ---- unet_ref.forward without its detach(): a function of x that torch.func.jvp can differentiate -----------------------------------------------

def forward_fn(state_dict, sigma, aug_cond=None, dtype=F64):
    """x -> F(x, sigma): the top-level walk of ``unet_ref.forward`` over ``ur._block`` / ``ur._sd``, sigma and the conditioning held fixed."""
    wrapped = any(k.startswith("inner_model.") for k in state_dict)
    sd = ur._sd(state_dict, dtype)
    sigma = sigma.detach().to(dtype).reshape(-1)
    f = 2 * math.pi * (sigma.log() / 4)[:, None] @ sd["timestep_embed.weight"].T
    emb = torch.cat([f.cos(), f.sin()], dim=-1)
    if wrapped:
        cond_in = emb.new_zeros(sigma.shape[0], 9) if aug_cond is None else aug_cond.detach().to(dtype)
        emb = emb + F.linear(cond_in, sd["mapping_cond.weight"])
    h = F.gelu(F.linear(emb, sd["mapping.0.weight"], sd["mapping.0.bias"]))
    cond = F.gelu(F.linear(h, sd["mapping.2.weight"], sd["mapping.2.bias"]))
    n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("u_net.d_blocks."))

    def fn(x):
        h = F.conv2d(x, sd["proj_in.weight"], sd["proj_in.bias"])
        skips = []
        for i in range(n):
            h = ur._block(sd, f"u_net.d_blocks.{i}.", h, cond)
            skips.append(h)
        for k in range(n):
            if k > 0:
                h = torch.cat([h, skips[n - 1 - k]], dim=1)
            h = ur._block(sd, f"u_net.u_blocks.{k}.", h, cond)
        return F.conv2d(h, sd["proj_out.weight"], sd["proj_out.bias"])
    return fn


def denoiser_fn(state_dict, sigma, sigma_data, aug_cond=None, dtype=F64):
    """x -> D(x, sigma) = F(x c_in) c_out + x c_skip (``unet_ref.denoiser``'s scalings) over ``forward_fn``."""
    fn = forward_fn(state_dict, sigma, aug_cond, dtype)
    s = sigma.detach().to(dtype).reshape(-1)
    var = s ** 2 + sigma_data ** 2
    c_skip, c_out, c_in = (t[:, None, None, None] for t in (sigma_data ** 2 / var, s * sigma_data / var.sqrt(), 1 / var.sqrt()))
    return lambda x: fn(x * c_in) * c_out + x * c_skip


@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_restated_walk_is_the_restatement(name):
    cfg, _, sd = built(name)
    x, sigma, aug = ur.inputs(name)
    assert torch.equal(forward_fn(sd, sigma, aug)(x.double()), ur.forward(sd, x, sigma, aug_cond=aug))
    sdata = cfg["model"]["sigma_data"]
    kw = {} if aug is None else {"aug_cond": aug}
    assert torch.equal(denoiser_fn(sd, sigma, sdata, aug)(x.double()), ur.denoiser(sd, sdata)(x, sigma, **kw))


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------------

def test_signatures_and_header_agree_for_the_dual_entry_points(KD):
    from tests.test_host_cpu import header_prototypes
    protos = header_prototypes()
    nat = KD._native
    for name, n_args in NEW_ENTRY_POINTS.items():
        assert protos[name] == n_args == len(nat.SIGNATURES[name]), name
        assert nat.SIGNATURES[name][-1] is C.c_void_p and name not in nat.RUN_LIST_OPS
        assert hasattr(nat.lib(), name)
    assert protos["kd_conv2d_x3"] == 15 == len(nat.SIGNATURES["kd_conv2d_x3"])
    assert nat.SIGNATURES["kd_conv2d_x3_stacked"] == nat.SIGNATURES["kd_conv2d_x3"][:-1] + [C.c_int, C.c_void_p]     # bias_batch in front of stream
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "kdiff_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        kinds = [C.c_void_p if "*" in a else (C.c_float if a.strip().startswith("float") else C.c_int) for a in decl.split(",")]
        assert kinds == nat.SIGNATURES[name], name
    assert all(callable(getattr(KD.unet_ops, n)) for n in ("groupnorm_stats_jvp", "adagn_apply_jvp"))
    assert not {"groupnorm_stats_jvp", "adagn_apply_jvp"} & set(vars(KD.ops))


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ur.CONFIGS))
def test_forward_jvp_refusals_without_a_device(KD, name):
    _, model, _ = built(name)
    x, sigma, aug = ur.inputs(name)
    kw = {} if aug is None else {"aug_cond": aug}
    with torch.no_grad():
        for call in (model.forward_jvp, KD.Denoiser(model, 0.5).forward_jvp):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(x, sigma, torch.ones_like(x), **kw)
            with pytest.raises(ValueError, match="tangent"):
                call(x, sigma, torch.ones_like(x)[:1], **kw)
            with pytest.raises(ValueError, match="tangent"):
                call(x, sigma, None, **kw)
    with pytest.raises(NotImplementedError, match="image_v1: sampling only"):
        model.forward_jvp(x, sigma, torch.ones_like(x).requires_grad_(True), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.likelihood.log_likelihood(KD.Denoiser(model, 0.5), x, 0.01, 80.0)

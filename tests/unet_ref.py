"""An independent restatement of the image_v1 U-Net's forward (k_diffusion/models/image_v1.py, layers.py:162-312) as plain functions of a
state dict, in torch on the CPU and in whatever dtype the inputs have (fp64 for truth, fp32 to measure fp32's own error).  NCHW throughout,
``F.group_norm`` / ``F.conv2d`` / ``F.conv_transpose2d`` as the reference calls them, attention spelt out as softmax(q k^T / 8) v: it shares nothing
with the kernels' token-major decomposition.  Also the two tiny configs of the tests and their seeded inputs.
"""
import math

import torch
from torch.nn import functional as F

UNET_A = {"model": {"type": "image_v1", "input_channels": 3, "input_size": [12, 20], "mapping_out": 64, "depths": [1, 2], "channels": [64, 128],
                    "self_attn_depths": [False, True], "augment_wrapper": True, "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80},
          "dataset": {"type": "imagefolder", "num_classes": 0}}
UNET_B = {"model": {"type": "image_v1", "input_channels": 1, "input_size": [28, 28], "mapping_out": 64, "depths": [1, 1, 1], "channels": [64, 64, 128],
                    "self_attn_depths": [False, False, True], "augment_wrapper": False, "sigma_data": 0.5, "sigma_min": 1e-2, "sigma_max": 80},
          "dataset": {"type": "imagefolder", "num_classes": 0}}
CONFIGS = {"unet_a": UNET_A, "unet_b": UNET_B}
SIGMAS = {"unet_a": [0.02, 1.5, 70.0], "unet_b": [0.3, 12.0]}
SEED = 11
USE_SDPA = False         # benchmarks/unet_bench.py: attention through F.scaled_dot_product_attention (what the reference calls) instead of spelt out


def inputs(name):
    """(x [B, C, H, W], sigma [B], aug_cond [B, 9] or None) of a tiny config, fp32 on the CPU, from seeds."""
    m = CONFIGS[name]["model"]
    g = torch.Generator().manual_seed(1000 + len(name) + m["input_channels"])
    sigma = torch.tensor(SIGMAS[name], dtype=torch.float32)
    B = sigma.shape[0]
    x = torch.randn(B, m["input_channels"], *m["input_size"], generator=g) * (sigma ** 2 + m["sigma_data"] ** 2).sqrt()[:, None, None, None]
    aug = 0.5 * torch.randn(B, 9, generator=g) if m["augment_wrapper"] else None
    return x, sigma, aug


def _sd(state_dict, dtype, device="cpu"):
    strip = "inner_model."
    return {(k[len(strip):] if k.startswith(strip) else k): v.detach().to(device=device, dtype=dtype) for k, v in state_dict.items()}


def adagn(sd, p, x, cond, groups):
    w, b = F.linear(cond, sd[p + "mapper.weight"], sd[p + "mapper.bias"]).chunk(2, dim=-1)
    x = F.group_norm(x, groups, eps=1e-5)
    return torch.addcmul(b[:, :, None, None], x, w[:, :, None, None] + 1)


def res_block(sd, p, x, cond):
    c_in = x.shape[1]
    h = F.gelu(adagn(sd, p + "main.0.", x, cond, max(1, c_in // 32)))
    h = F.conv2d(h, sd[p + "main.2.weight"], sd[p + "main.2.bias"], padding=1)
    h = F.gelu(adagn(sd, p + "main.4.", h, cond, max(1, h.shape[1] // 32)))
    h = F.conv2d(h, sd[p + "main.6.weight"], sd[p + "main.6.bias"], padding=1)
    skip = F.conv2d(x, sd[p + "skip.weight"]) if p + "skip.weight" in sd else x
    return h + skip


def self_attention(sd, p, x, cond):
    n, c, h, w = x.shape
    nh = max(1, c // 64)
    qkv = F.conv2d(adagn(sd, p + "norm_in.", x, cond, max(1, c // 32)), sd[p + "qkv_proj.weight"], sd[p + "qkv_proj.bias"])
    qkv = qkv.view(n, nh * 3, c // nh, h * w).transpose(2, 3)
    q, k, v = qkv.chunk(3, dim=1)
    if USE_SDPA:
        att = F.scaled_dot_product_attention(q, k, v)
    else:
        att = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(q.shape[-1]), dim=-1) @ v
    y = att.transpose(2, 3).contiguous().view(n, c, h, w)
    return x + F.conv2d(y, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def _depthwise(x, kernel):
    """The reference's dense [C, C, 4, 4] weight with the kernel on its diagonal (layers.py:261-263)."""
    c = x.shape[1]
    weight = x.new_zeros(c, c, *kernel.shape)
    idx = torch.arange(c, device=x.device)
    weight[idx, idx] = kernel.to(x)
    return weight


def downsample(x, kernel, grouped=False):
    """layers.py:259-264 with the model's 'kernel' buffer.  ``grouped``: the same sum as a depthwise (groups = C) conv, for timing."""
    x = F.pad(x, (1,) * 4, "reflect")
    if grouped:
        return F.conv2d(x, kernel.to(x).expand(x.shape[1], 1, -1, -1), stride=2, groups=x.shape[1])
    return F.conv2d(x, _depthwise(x, kernel), stride=2)


def upsample(x, kernel, grouped=False):
    """layers.py:275-280."""
    x = F.pad(x, (1,) * 4, "reflect")
    if grouped:
        return F.conv_transpose2d(x, kernel.to(x).expand(x.shape[1], 1, -1, -1), stride=2, padding=3, groups=x.shape[1])
    return F.conv_transpose2d(x, _depthwise(x, kernel), stride=2, padding=3)


def _layers(sd, prefix):
    """The numbered children of a block that hold layers, in order: (index, kind)."""
    out, i = [], 0
    seen = {k[len(prefix):].split(".")[0] for k in sd if k.startswith(prefix)}
    for i in sorted(int(s) for s in seen):
        p = f"{prefix}{i}."
        if p + "main.2.weight" in sd:
            out.append((p, "res"))
        elif p + "qkv_proj.weight" in sd:
            out.append((p, "attn"))
        elif p + "kernel" in sd:
            out.append((p, "resample"))
    return out


def _block(sd, prefix, x, cond, grouped=False):
    for p, kind in _layers(sd, prefix):
        if kind == "res":
            x = res_block(sd, p, x, cond)
        elif kind == "attn":
            x = self_attention(sd, p, x, cond)
        elif prefix.startswith("u_net.d_blocks"):
            x = downsample(x, sd[p + "kernel"], grouped)
        else:
            x = upsample(x, sd[p + "kernel"], grouped)
    return x


def forward(state_dict, x, sigma, aug_cond=None, mapping_cond=None, dtype=torch.float64, device="cpu", grouped_resample=False, prepared=False):
    """F(x, sigma) of the (possibly augment-wrapped) model whose weights are ``state_dict``.  A wrapped model (keys under ``inner_model.``)
    gets zeros [B, 9] for a missing ``aug_cond``, as KarrasAugmentWrapper does.  ``device`` / ``grouped_resample`` / ``prepared`` (the state
    dict is already ``prepare``d: no per-call conversion) serve benchmarks/unet_bench.py, which times this as plain torch on the GPU."""
    wrapped = any(k.startswith("inner_model.") for k in state_dict) or bool(state_dict.get("__wrapped__", False))
    sd = state_dict if prepared else _sd(state_dict, dtype, device)
    to = lambda t: t.detach().to(device=device, dtype=dtype)
    x, sigma = to(x), to(sigma).reshape(-1)
    cond_in = None
    if wrapped:
        cond_in = x.new_zeros(x.shape[0], 9) if aug_cond is None else to(aug_cond)
        if mapping_cond is not None:
            cond_in = torch.cat([cond_in, to(mapping_cond)], dim=1)
    elif mapping_cond is not None:
        cond_in = to(mapping_cond)
    f = 2 * math.pi * (sigma.log() / 4)[:, None] @ sd["timestep_embed.weight"].T
    emb = torch.cat([f.cos(), f.sin()], dim=-1)
    if cond_in is not None:
        emb = emb + F.linear(cond_in, sd["mapping_cond.weight"])
    h = F.gelu(F.linear(emb, sd["mapping.0.weight"], sd["mapping.0.bias"]))
    cond = F.gelu(F.linear(h, sd["mapping.2.weight"], sd["mapping.2.bias"]))
    h = F.conv2d(x, sd["proj_in.weight"], sd["proj_in.bias"])
    n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("u_net.d_blocks."))
    skips = []
    for i in range(n):
        h = _block(sd, f"u_net.d_blocks.{i}.", h, cond, grouped_resample)
        skips.append(h)
    for k in range(n):
        if k > 0:
            h = torch.cat([h, skips[n - 1 - k]], dim=1)
        h = _block(sd, f"u_net.u_blocks.{k}.", h, cond, grouped_resample)
    return F.conv2d(h, sd["proj_out.weight"], sd["proj_out.bias"])


def prepare(state_dict, dtype, device):
    """The state dict as ``forward(..., prepared=True)`` takes it: prefix stripped, on ``device`` in ``dtype``, the wrapper remembered."""
    sd = _sd(state_dict, dtype, device)
    sd["__wrapped__"] = any(k.startswith("inner_model.") for k in state_dict)
    return sd


def denoiser(state_dict, sigma_data, dtype=torch.float64):
    """D(x, sigma, **kwargs) = F(x c_in) c_out + x c_skip (layers.py:70-74, 88-90) over ``forward``."""
    def den(x, sigma, **kwargs):
        x, sigma = x.to(dtype), sigma.to(dtype).reshape(-1)
        var = sigma ** 2 + sigma_data ** 2
        c_skip, c_out, c_in = (t[:, None, None, None] for t in (sigma_data ** 2 / var, sigma * sigma_data / var.sqrt(), 1 / var.sqrt()))
        return forward(state_dict, x * c_in, sigma, dtype=dtype, **kwargs) * c_out + x * c_skip
    return den

"""Shared by the dropout tests of the image_v1 U-Net and by tests/golden/make_golden_unet_drop.py: the forward of tests/unet_ref.py restated with
INJECTED dropout masks -- one [B, C] mask behind each convolution of a residual block (the reference's nn.Dropout2d, image_v1.py:22,26: whole
(sample, channel) maps; the first sits in front of the second AdaGN, whose statistics see it, the second between conv2 + bias and the residual
add) and one [B, nh, T, T] mask on the softmax probabilities of each attention layer (F.scaled_dot_product_attention(dropout_p=p),
layers.py:196; nothing behind out_proj) -- the training loss over it, and a numpy statement of the kernels' mask contract
(include/kdiff_unet_drop.h) on ``oracle.brownian.philox4x32_10``.

A mask here is a tensor of KEEP flags (1 kept, 0 dropped); the restatement multiplies by mask / (1 - p).  Masks are consumed in the order the
forward reaches their sites: per layer in ``image_v1.forward_layers`` order, a residual block's two, then an attention layer's one.
"""
import math

import numpy as np
import torch
from torch.nn import functional as F

from oracle.brownian import philox4x32_10
from tests import unet_ref as ur
from tests import unet_train_ref as tr

RATE = 0.25                      # the dropout rate of the golden and of the model-level GPU tests
SITE = 1 << 62 | 1 << 33         # the bits every site id of this family carries


# ---- the mask contract in numpy ------------------------------------------------------------------------------------------------------------------

def keep_flags(key, site, p, n):
    """keep[e] for e < n at ``site`` under ``key`` (any Python int; taken mod 2^64): word e & 3 of philox4x32_10(key, counter (e >> 2, site))
    >= floor(p 2^32)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10(key & (2 ** 64 - 1), q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), site & 0xFFFFFFFF, site >> 32)
    w = np.stack(np.broadcast_arrays(*words), axis=1).reshape(-1)[:n]
    return w >= np.uint32(int(math.floor(p * 2.0 ** 32)))


def scale_of(p):
    """(float)(1 / (1 - p)), the division in double."""
    return np.float32(1.0 / (1.0 - p))


def chan_keep(key, site, p, B, C):
    """[B, C] keep flags of a channel site: element e = b C + c."""
    return keep_flags(key, site, p, B * C).reshape(B, C)


def attn_keep(key, site, p, B, nh, T):
    """[B, nh, T, T] keep flags of an attention site: element e = ((b nh + h) T + i) T4 + j with T4 = 4 ceil(T / 4) -- the padding columns
    j >= T of every row are drawn and thrown away."""
    T4 = 4 * -(-T // 4)
    return keep_flags(key, site, p, B * nh * T * T4).reshape(B, nh, T, T4)[..., :T]


def site_list(sd):
    """[(site id, kind, prefix)] in forward order from a state dict of the (unwrapped) model: kind "conv1" / "conv2" / "attn"."""
    sd = {(k[len("inner_model."):] if k.startswith("inner_model.") else k): v for k, v in sd.items()}
    n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("u_net.d_blocks."))
    out, L = [], 0
    for prefix in [f"u_net.d_blocks.{i}." for i in range(n)] + [f"u_net.u_blocks.{k}." for k in range(n)]:
        for p, kind in ur._layers(sd, prefix):
            if kind == "res":
                out += [(SITE | 2 * L, "conv1", p), (SITE | (2 * L + 1), "conv2", p)]
            elif kind == "attn":
                out.append((SITE | 2 * L, "attn", p))
            else:
                continue
            L += 1
    return out


def philox_masks(sd, key, p, B, hw):
    """The keep masks (torch bool, forward order) the kernels draw for a loss call with ``key`` on a batch of B images of size ``hw``."""
    sd = {(k[len("inner_model."):] if k.startswith("inner_model.") else k): v for k, v in sd.items()}
    masks = []
    for site, kind, prefix in site_list(sd):
        level = int(prefix.split(".")[2])
        if prefix.startswith("u_net.u_blocks."):
            n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("u_net.d_blocks."))
            level = n - 1 - level
        if kind == "attn":
            C = sd[prefix + "out_proj.weight"].shape[0]
            T = (hw[0] >> level) * (hw[1] >> level)
            masks.append(torch.from_numpy(attn_keep(key, site, p, B, max(1, C // 64), T)))
        else:
            C = sd[prefix + ("main.2.weight" if kind == "conv1" else "main.6.weight")].shape[0]
            masks.append(torch.from_numpy(chan_keep(key, site, p, B, C)))
    return masks


# ---- masks as the golden stores them -----------------------------------------------------------------------------------------------------------------

def pack(mask):
    """{"shape": [...], "bits": hex}: the keep flags, row-major, most significant bit first, padded with zeros to a byte."""
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    return {"shape": list(m.shape), "bits": np.packbits(m.reshape(-1)).tobytes().hex()}


def unpack(rec):
    n = int(np.prod(rec["shape"]))
    bits = np.unpackbits(np.frombuffer(bytes.fromhex(rec["bits"]), dtype=np.uint8))[:n]
    return torch.from_numpy(bits.astype(bool).reshape(rec["shape"]))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------

def res_block(sd, p, x, cond, m1, m2, rate):
    c_in = x.shape[1]
    s = 1.0 / (1.0 - rate)
    h = F.gelu(ur.adagn(sd, p + "main.0.", x, cond, max(1, c_in // 32)))
    h = F.conv2d(h, sd[p + "main.2.weight"], sd[p + "main.2.bias"], padding=1)
    h = h * (m1.to(h) * s)[:, :, None, None]
    h = F.gelu(ur.adagn(sd, p + "main.4.", h, cond, max(1, h.shape[1] // 32)))
    h = F.conv2d(h, sd[p + "main.6.weight"], sd[p + "main.6.bias"], padding=1)
    h = h * (m2.to(h) * s)[:, :, None, None]
    skip = F.conv2d(x, sd[p + "skip.weight"]) if p + "skip.weight" in sd else x
    return h + skip


def self_attention(sd, p, x, cond, m, rate):
    n, c, h, w = x.shape
    nh = max(1, c // 64)
    qkv = F.conv2d(ur.adagn(sd, p + "norm_in.", x, cond, max(1, c // 32)), sd[p + "qkv_proj.weight"], sd[p + "qkv_proj.bias"])
    qkv = qkv.view(n, nh * 3, c // nh, h * w).transpose(2, 3)
    q, k, v = qkv.chunk(3, dim=1)
    prob = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(q.shape[-1]), dim=-1)
    att = (prob * (m.to(prob) * (1.0 / (1.0 - rate)))) @ v
    y = att.transpose(2, 3).contiguous().view(n, c, h, w)
    return x + F.conv2d(y, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def forward(sd, x, sigma, masks, rate=RATE, aug_cond=None, dtype=torch.float64):
    """``unet_ref.forward`` with the keep masks ``masks`` (forward order) at rate ``rate``.  ``sd``: the state dict in ``dtype`` already
    (tensors that require grad keep their graph), under the wrapper's ``inner_model.`` prefix or not."""
    wrapped = any(k.startswith("inner_model.") for k in sd)
    sd = {(k[len("inner_model."):] if k.startswith("inner_model.") else k): v for k, v in sd.items()}
    x, sigma = x.to(dtype), sigma.to(dtype).reshape(-1)
    masks = iter(masks)
    cond_in = None
    if wrapped:
        cond_in = x.new_zeros(x.shape[0], 9) if aug_cond is None else aug_cond.to(dtype)
    f = 2 * math.pi * (sigma.log() / 4)[:, None] @ sd["timestep_embed.weight"].T
    emb = torch.cat([f.cos(), f.sin()], dim=-1)
    if cond_in is not None:
        emb = emb + F.linear(cond_in, sd["mapping_cond.weight"])
    cond = F.gelu(F.linear(F.gelu(F.linear(emb, sd["mapping.0.weight"], sd["mapping.0.bias"])), sd["mapping.2.weight"], sd["mapping.2.bias"]))
    h = F.conv2d(x, sd["proj_in.weight"], sd["proj_in.bias"])
    n = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("u_net.d_blocks."))

    def block(prefix, h):
        for p, kind in ur._layers(sd, prefix):
            if kind == "res":
                h = res_block(sd, p, h, cond, next(masks), next(masks), rate)
            elif kind == "attn":
                h = self_attention(sd, p, h, cond, next(masks), rate)
            elif prefix.startswith("u_net.d_blocks"):
                h = ur.downsample(h, sd[p + "kernel"])
            else:
                h = ur.upsample(h, sd[p + "kernel"])
        return h
    skips = []
    for i in range(n):
        h = block(f"u_net.d_blocks.{i}.", h)
        skips.append(h)
    for k in range(n):
        if k > 0:
            h = torch.cat([h, skips[n - 1 - k]], dim=1)
        h = block(f"u_net.u_blocks.{k}.", h)
    assert next(masks, None) is None, "more masks than sites"
    return F.conv2d(h, sd["proj_out.weight"], sd["proj_out.bias"])


def losses(sd, x, noise, sigma, aug, weighting, masks, rate=RATE, dtype=torch.float64, sigma_data=tr.SIGMA_DATA):
    """``unet_train_ref.losses`` over the masked forward: per-sample losses [B]."""
    x, noise, sigma = (t.to(dtype) for t in (x, noise, sigma))
    var = sigma ** 2 + sigma_data ** 2
    c_skip, c_out, c_in = (t[:, None, None, None] for t in (sigma_data ** 2 / var, sigma * sigma_data / var.sqrt(), 1 / var.sqrt()))
    noised = x + noise * sigma[:, None, None, None]
    f = forward(sd, noised * c_in, sigma, masks, rate, aug, dtype)
    target = (x - c_skip * noised) / c_out
    return (f - target).pow(2).flatten(1).mean(1) * tr.c_weight(weighting, sigma, sigma_data)


def dropping_config(name, rate=RATE):
    """The tiny config ``name`` of tests/unet_ref.py with ``dropout_rate`` = rate."""
    import json
    raw = json.loads(json.dumps(ur.CONFIGS[name]))
    raw["model"]["dropout_rate"] = rate
    return raw

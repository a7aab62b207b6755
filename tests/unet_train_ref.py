"""Shared by the training tests of the image_v1 U-Net and by tests/golden/make_golden_unet_train.py: the seeded batch of a tiny config of
tests/unet_ref.py, the probe vector of the golden, and the loss of ``Denoiser.loss`` (k_diffusion/layers.py:64-86) restated over
``unet_ref.forward`` -- plain torch in the dtype it is handed, differentiable w.r.t. a state dict's tensors by autograd."""
import torch

from tests import unet_ref as ur

SIGMA_DATA = 0.5
WEIGHTINGS = ("karras", "soft-min-snr", "snr")


def batch(name):
    """(input, noise, sigma, aug_cond or None): the clean images, the noise and the noise levels of one training step, fp32 from seeds."""
    m = ur.CONFIGS[name]["model"]
    g = torch.Generator().manual_seed(2000 + len(name) + m["input_channels"])
    sigma = torch.tensor(ur.SIGMAS[name], dtype=torch.float32)
    B = sigma.shape[0]
    x = SIGMA_DATA * torch.randn(B, m["input_channels"], *m["input_size"], generator=g)
    noise = torch.randn(x.shape, generator=g)
    aug = 0.5 * torch.randn(B, 9, generator=g) if m["augment_wrapper"] else None
    return x, noise, sigma, aug


def probe(numel, dtype=torch.float64):
    return torch.cos(0.37 * torch.arange(numel, dtype=dtype) + 1)


def c_weight(weighting, sigma, sigma_data=SIGMA_DATA):
    if callable(weighting):
        return weighting(sigma)
    if weighting == "karras":
        return torch.ones_like(sigma)
    if weighting == "soft-min-snr":
        return (sigma * sigma_data) ** 2 / (sigma ** 2 + sigma_data ** 2) ** 2
    if weighting == "snr":
        return sigma_data ** 2 / (sigma ** 2 + sigma_data ** 2)
    raise ValueError(weighting)


def losses(sd, x, noise, sigma, aug, weighting, dtype=torch.float64, sigma_data=SIGMA_DATA, device="cpu"):
    """Per-sample losses [B] of the model whose weights are ``sd`` (tensors of ``dtype``; those that require grad get one)."""
    x, noise, sigma = (t.to(device=device, dtype=dtype) for t in (x, noise, sigma))
    var = sigma ** 2 + sigma_data ** 2
    c_skip, c_out, c_in = (t[:, None, None, None] for t in (sigma_data ** 2 / var, sigma * sigma_data / var.sqrt(), 1 / var.sqrt()))
    noised = x + noise * sigma[:, None, None, None]
    f = forward_keep_graph(sd, noised * c_in, sigma, aug, dtype, device)
    target = (x - c_skip * noised) / c_out
    return (f - target).pow(2).flatten(1).mean(1) * c_weight(weighting, sigma, sigma_data)


def forward_keep_graph(sd, x, sigma, aug, dtype, device="cpu"):
    """``unet_ref.forward`` on a state dict that is already in ``dtype`` on ``device`` and may require grad (``prepared``: no detach)."""
    wrapped = any(k.startswith("inner_model.") for k in sd)
    prepared = {(k[len("inner_model."):] if k.startswith("inner_model.") else k): v for k, v in sd.items()}
    prepared["__wrapped__"] = wrapped
    return ur.forward(prepared, x, sigma, aug_cond=aug, dtype=dtype, device=device, prepared=True)


def leaf_state(sd, names, dtype=torch.float64, device="cpu"):
    """The state dict in ``dtype`` with the entries ``names`` (parameter names) as leaves that require grad."""
    return {k: v.detach().to(device=device, dtype=dtype).requires_grad_(k in names) for k, v in sd.items()}


def summary(grad):
    """(L2 norm, inner product with the probe) of one gradient, as the golden records them."""
    g = grad.detach().double().cpu().reshape(-1)
    return [g.norm().item(), torch.dot(g, probe(g.numel())).item()]

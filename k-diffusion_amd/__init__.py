"""MI355X-native k-diffusion sampling hot path.

``import k_diffusion_amd as K`` mirrors ``import k_diffusion as K`` for the sampling path:
K.sampling, K.layers / K.Denoiser, K.config, K.models, K.evaluation, K.utils (+ K.distributed,
K.ops, K.synth, K.likelihood (log_likelihood on a forward-mode JVP of the denoiser), K.optim (the fused clip + AdamW + EMA step), K.training (make_sample_density), K.augmentation (the Karras augmentation pipeline as a batched device op), K.unet_ops (the tensor-level wrappers of the image_v1 U-Net's kernels), K.data (labelled datasets: CIFAR-10 / MNIST resident on the device, class folders, conditioning dropout), and K.compat: natten's na2d / flash-attn's packed call / SDPA under their own signatures on the HIP cores).  Importing the package never needs a GPU; the first kernel call loads
csrc/libkdiff_hip.so and fails loudly if it is missing (there is no CPU fallback).
"""
from . import _native, augmentation, checkpoint, compat, config, data, distributed, evaluation, external, layers, likelihood, models, ops, optim, sampling, synth, training, unet_ops, utils  # noqa: F401
from .layers import Denoiser  # noqa: F401

__version__ = "0.1.0"

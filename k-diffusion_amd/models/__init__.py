"""Denoiser networks on the MI355X hot path: the hourglass transformer (image_transformer_v2; sampling, likelihood and training) and the
reference's U-Net (image_v1; sampling, likelihood, input gradients and the training loss's parameter gradients).  The transformer v1 family is out of scope."""
from . import axial_rope, flops, image_transformer_v2, image_v1  # noqa: F401
from .image_transformer_v2 import ImageTransformerDenoiserModelV2  # noqa: F401
from .image_v1 import ImageDenoiserModelV1  # noqa: F401

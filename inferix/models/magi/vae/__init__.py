"""inferix/models/magi/vae: the decode side of the MAGI ViT-VAE (`ViTVAE.decode`, `ViTDecoder`) on the HIP kernels; the encoder, `AutoModel`
checkpoint loading and `DiagonalGaussianDistribution` are not built."""
from .vae_model import ViTVAE  # noqa: F401
from .vae_module import ViTDecoder  # noqa: F401

__all__ = ["ViTVAE", "ViTDecoder"]

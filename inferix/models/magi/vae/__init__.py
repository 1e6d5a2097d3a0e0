"""inferix/models/magi/vae: the MAGI ViT-VAE (`ViTVAE.encode` / `.decode` and their tiled forms, `ViTEncoder`, `ViTDecoder`) on the HIP
kernels; `AutoModel` checkpoint loading and the `DiagonalGaussianDistribution` class are not built (sampling is a method of `ViTVAE`)."""
from .vae_model import ViTVAE  # noqa: F401
from .vae_module import ViTDecoder, ViTEncoder  # noqa: F401

__all__ = ["ViTVAE", "ViTDecoder", "ViTEncoder"]

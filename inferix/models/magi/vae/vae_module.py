"""inferix/models/magi/vae/vae_module.py: ViTDecoder :569-716 (Attention :261-301, Block :307-346, ManualLayerNorm :229-242)"""
from inferix_amd.magi.vae import HipViTDecoder as ViTDecoder  # noqa: F401

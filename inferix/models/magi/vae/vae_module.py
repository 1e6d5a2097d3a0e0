"""inferix/models/magi/vae/vae_module.py: ViTEncoder :409-558 (PatchEmbed :352-394), ViTDecoder :569-716 (Attention :261-301,
Block :307-346, ManualLayerNorm :229-242)"""
from inferix_amd.magi.vae import HipViTDecoder as ViTDecoder  # noqa: F401
from inferix_amd.magi.vae import HipViTEncoder as ViTEncoder  # noqa: F401

"""inferix/models/magi/vae/vae_model.py: ViTVAE :222-329 (decode :290-308; encode raises NotImplementedError)"""
from inferix_amd.magi.vae import HipMagiVAEDecoder as ViTVAE  # noqa: F401

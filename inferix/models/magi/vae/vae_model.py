"""inferix/models/magi/vae/vae_model.py: ViTVAE :222-329 (encode :259-288, decode :290-308, tiled_encode_3d :137-177,
tiled_decode_3d :179-219; the encode side needs encoder weights in the loaded state dict)"""
from inferix_amd.magi.vae import HipMagiVAEDecoder as ViTVAE  # noqa: F401

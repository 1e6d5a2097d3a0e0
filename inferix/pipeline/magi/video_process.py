"""inferix/pipeline/magi/video_process.py: VaeHelper.decode :155-200 (tiled chunk decode + the uint8 tail; get_vae and encode are not
built: they load a checkpoint / run the encoder)"""
from inferix_amd.magi.vae import VaeHelper  # noqa: F401

"""inferix/pipeline/magi/video_process.py: VaeHelper.encode :113-153 (tiled prefix-video encode, every tile the posterior's mode),
VaeHelper.decode :155-200 (tiled chunk decode + the uint8 tail), encode_prefix_video :279-312 (with the vae object in place of the
checkpoint path).  get_vae loads a checkpoint and the ffmpeg readers decode files: both stay with the caller."""
from inferix_amd.magi.vae import VaeHelper, encode_prefix_video  # noqa: F401

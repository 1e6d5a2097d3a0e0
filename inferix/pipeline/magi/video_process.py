"""inferix/pipeline/magi/video_process.py: VaeHelper.encode :113-153 (tiled prefix-video encode, every tile the posterior's mode),
VaeHelper.decode :155-200 (tiled chunk decode + the uint8 tail), encode_prefix_video :279-312 (with the vae object in place of the
checkpoint path), decode_chunk :348-374 and post_chunk_process :377-388 (`post_chunk_process(chunk, config, vae)`: the vae object again).
get_vae loads a checkpoint and the ffmpeg readers decode files: both stay with the caller."""
from inferix_amd.magi.vae import VaeHelper, decode_chunk, encode_prefix_video, post_chunk_process  # noqa: F401

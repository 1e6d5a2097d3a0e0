"""MagiPipeline — the outer plugin API of a MAGI request (BASELINE config 5, PER_BLOCK decode).

Mirror of `inferix.pipeline.magi.pipeline.MagiPipeline` (pipeline/magi/pipeline.py:32-114) on `AbstractInferencePipeline`:
`run_text_to_video`, `run_image_to_video`, `run_video_to_video` (the last two encode their pixels with `encode_prefix_video` first, as
upstream's `process_image` / `process_prefix_video` do), `_run` = `get_txt_embeddings` -> `generate_per_chunk` -> `post_chunk_process`
per chunk as it arrives -> `torch.cat` -> the writer.  What differs:

  * the parts are injected: the constructor takes the config OBJECT (`model_config` / `engine_config` / `runtime_config`, as
    `MagiConfig` carries them) and `dit` (`HipVideoDiTModel`), `vae` (`HipMagiVAEDecoder`), `embedder` (`HipT5Embedder`) — upstream
    reads a json, calls `dist_init` and loads three checkpoints per request; loading, process groups and the ffmpeg readers and
    writers stay with the caller;
  * the pixels of an image or a prefix video come in as tensors (`image=` uint8 `[1, H, W, 3]`, `prefix_video=` uint8 `[T, H, W, 3]`,
    what upstream's `ffmpeg_i2v` / `ffmpeg_v2v` return); a path without the tensor is an error that names the keyword;
  * the frames are RETURNED (`[T, 3, H, W]` uint8 on the device); `writer(frames, output_path, fps)`, if one was given, stands where
    upstream's `save_video_to_disk` does.

Each chunk is decoded on the stream that denoises, between two forwards, as upstream does it.

`run_streaming_generation` / `run_interactive_generation(..., continuous=True)` (not upstream) stream a request: every chunk
is pushed into one `MagiFrameStream` the moment it is handed out, its frames finished as uint8 `[T', H', W', 3]` by the tile blend and
copied to the host behind the denoising loop; `_run` and the three `run_*_to_video` methods are as they were.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch

from ..magi.prompt import get_txt_embeddings
from ..magi.schedule import generate_per_chunk
from ..magi.vae import encode_prefix_video, post_chunk_process
from .base_pipeline import AbstractInferencePipeline


class MagiPipeline(AbstractInferencePipeline):
    def __init__(self, config, *, dit, vae, embedder, writer: Optional[Callable[[torch.Tensor, str, int], None]] = None,
                 profiling_config=None):
        self.magi_config = config
        self.dit, self.vae, self.embedder, self.writer = dit, vae, embedder, writer
        AbstractInferencePipeline.__init__(self, config, profiling_config)

    def _initialize_pipeline(self):
        """Nothing to do: the parts arrive built."""

    def load_checkpoint(self, checkpoint_path: str, **kwargs) -> None:
        """Nothing to do, as upstream: the injected parts carry their weights."""

    # ------------------------------------------------------------------------------------------------------
    def run_text_to_video(self, prompt: str, output_path: Optional[str] = None, **kwargs) -> torch.Tensor:
        return self._run(prompt, None, output_path or "./output.mp4")

    def run_image_to_video(self, prompt: str, image_path: Optional[str] = None, output_path: Optional[str] = None, *,
                           image: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """`image` uint8 `[1, H, W, 3]` at the config's video size (upstream's `ffmpeg_i2v(image_path, w, h)`)."""
        if image is None:
            raise RuntimeError(f"run_image_to_video: decoding {image_path!r} needs ffmpeg, which stays with the caller; pass "
                               "image=tensor uint8 [1, H, W, 3] instead")
        return self._run(prompt, self._encode(image), output_path or "./output.mp4")

    def run_video_to_video(self, prompt: str, prefix_video_path: Optional[str] = None, output_path: Optional[str] = None, *,
                           prefix_video: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """`prefix_video` uint8 `[T, H, W, 3]` at the config's video size and fps (upstream's `ffmpeg_v2v(path, fps, 32, w, h)`)."""
        if prefix_video is None:
            raise RuntimeError(f"run_video_to_video: decoding {prefix_video_path!r} needs ffmpeg, which stays with the caller; pass "
                               "prefix_video=tensor uint8 [T, H, W, 3] instead")
        return self._run(prompt, self._encode(prefix_video), output_path or "./output.mp4")

    def _encode(self, pixels: torch.Tensor) -> torch.Tensor:
        """uint8 frames `[T, H, W, 3]` -> the clean prefix latents (upstream's `process_image` / `process_prefix_video`, which also
        encode before `_run` is entered)."""
        rc = self.magi_config.runtime_config
        return encode_prefix_video(pixels, rc.fps, self.vae, rc.scale_factor)

    @torch.no_grad()
    def _run(self, prompt: str, prefix_video: Optional[torch.Tensor], output_path: str) -> torch.Tensor:
        """`prefix_video`: the prefix LATENTS `_encode` made, or None (text to video)."""
        config = self.magi_config
        rc = config.runtime_config
        caption_embs, emb_masks = get_txt_embeddings(prompt, config, self.embedder)
        frames = torch.cat([post_chunk_process(chunk, config, self.vae)
                            for chunk in generate_per_chunk(model=self.dit, prefix_video=prefix_video, caption_embs=caption_embs,
                                                            emb_masks=emb_masks)], dim=0)
        if self.writer is not None:
            self.writer(frames, output_path, rc.fps)
        return frames

    def _make_frame_stream(self, stream_callback, keep_video: bool = True, **kwargs):
        """The `MagiFrameStream` of a `continuous=True` call, on the injected HIP VAE."""
        from ..streaming import MagiFrameStream
        try:
            return MagiFrameStream(self.vae, self.magi_config, callback=stream_callback, keep=keep_video,
                                   pixel_format=kwargs.get("pixel_format", "rgb24"), matrix=kwargs.get("matrix", "bt601"),
                                   full_range=kwargs.get("full_range", False))
        except TypeError as exc:
            raise ValueError(f"continuous=True: {exc}") from exc

    @torch.no_grad()
    def _generate_segment_with_streaming(self, prompt: str, initial_latent: Optional[torch.Tensor],
                                         stream_callback: Optional[Callable[[torch.Tensor], None]], segment_length: int = 21,
                                         continuous: bool = False, frame_stream=None, keep_video: bool = True,
                                         **kwargs) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """Without `continuous=True` / a `frame_stream`: upstream's `NotImplementedError`.

        With them (not upstream) one request: `get_txt_embeddings` -> `generate_per_chunk` (`noise=` from the keywords when
        given) -> `frame_stream.push(chunk)` per hand-out, the frames reaching `stream_callback` as host uint8 `[T', H', W', 3]`.
        `initial_latent` `[1, T_o, C, h, w]` (the base class's layout: the last `overlap_frames` latent frames of the segment before)
        becomes the clean prefix latents `[1, C, T_o, h, w]` as they are — generator latents and `encode_prefix_video` latents are in
        one domain; `T_o` need not be a multiple of `chunk_width` (a chunk the prefix reaches into is handed out from the prefix's end).
        On the first segment only (`initial_latent is None`) `image=` uint8 `[1, H, W, 3]` / `prefix_video=` uint8 `[T, H, W, 3]` start
        from an encoded prefix, as `run_image_to_video` / `run_video_to_video`; later segments ignore them.  Prefix frames are never
        handed out, so no frame is delivered twice.

        The request's length is the config's (`runtime_config.num_frames`, which counts the prefix): `segment_length` does not resize
        it.  Other keywords are accepted and ignored, as upstream's `**kwargs`.

        -> (video, final latents `[1, T_new, C, h, w]`: the handed-out chunks, concatenated).  With a `frame_stream` of the caller's
        the frames are still in flight when the segment returns, so the video is None and the caller collects it
        (`frame_stream.video()`); without one the segment opens its own stream, flushes it and returns this segment's frames as uint8
        `[1, T, H, W, 3]` (None with `keep_video=False`)."""
        fmt = self._pixel_format_kwargs(kwargs, continuous or frame_stream is not None)
        if not continuous and frame_stream is None:
            raise NotImplementedError("Streaming generation is not yet implemented for MagiPipeline. "
                                      "Please use the standard run_text_to_video or run_image_to_video methods.")
        config = self.magi_config
        own_stream = frame_stream is None
        if own_stream:
            frame_stream = self._make_frame_stream(stream_callback, keep_video, **fmt)
        else:
            self._check_stream_format(frame_stream, fmt)
        if initial_latent is not None:
            prefix = initial_latent.transpose(1, 2).contiguous()
        elif kwargs.get("image") is not None:
            prefix = self._encode(kwargs["image"])
        elif kwargs.get("prefix_video") is not None:
            prefix = self._encode(kwargs["prefix_video"])
        else:
            prefix = None
        caption_embs, emb_masks = get_txt_embeddings(prompt, config, self.embedder)
        chunks = []
        try:
            noise = {"noise": kwargs["noise"]} if kwargs.get("noise") is not None else {}
            for chunk in generate_per_chunk(model=self.dit, prefix_video=prefix, caption_embs=caption_embs, emb_masks=emb_masks, **noise):
                frame_stream.push(chunk)
                chunks.append(chunk)
        finally:
            if own_stream:
                frame_stream.flush()
        final_latents = torch.cat(chunks, dim=2).transpose(1, 2)
        video = frame_stream.video() if own_stream and keep_video else None
        return video, final_latents

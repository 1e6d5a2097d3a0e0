"""`FrameStream`: one continuous VAE stream per sample, uint8 frames finished on the device, handed to the consumer without stalling
the denoising loop.  `MagiFrameStream`: the same delivery for the chunks a MAGI request hands out.

The per-block streaming callback of the reference (pipeline/self_forcing/pipeline.py:700-760) decodes every block as a clip of its own
(`decode_to_pixel` clears the feature cache before and after), finishes the frames in fp32 and fetches them with a synchronous copy.
Here the decoder stream of a sample is opened once and never reset — the HIP decoder gives the same bits however its input is chunked,
so the frames are those of the one-shot decode of all latents pushed so far: `4 nf - 3` frames for the block that opens the stream,
`4 nf` for every later one, no seam at a block or segment boundary — and a block travels as

    current stream:  cached_decode_u8 (convs ... ifx_frames_u8 -> uint8 [T, H, W, 3])   event `decoded`
    copy stream:     wait(decoded); uint8 device -> pinned host, asynchronous            event `copied`
    host:            poll(): `copied` done?  read the device-error word, then callback(frames)

`push` never synchronises the host unless all `slots` buffers are in flight; then it waits for the oldest one (back-pressure: device
and pinned memory are `slots` blocks, however long the stream).  Everything runs on the calling thread.

Both streams share `_SlotStream` — the ring of slots, the copy stream with its two events per slot, `poll` / `flush` / `_deliver`,
`keep` / `video()` / `frames_pushed` / `timing` — and differ in `push` alone: what is decoded, and how, into the slot's device buffer.

`pixel_format="yuv420p"` / `"nv12"` (default `"rgb24"`): the frames leave the device as YUV 4:2:0, what a video encoder takes — the
integer conversion of include/inferix_hip.h (`matrix=` "bt601" / "bt709", `full_range=`), box-filtered chroma sited at the centre of
each 2 x 2 quad.  A block is then uint8 `[T, H * 3 / 2, W]` (`yuv420p`: Y, U, V planes per frame, the ndarray
`av.VideoFrame.from_ndarray(frame, format="yuv420p")` takes; `nv12`: Y, then interleaved UV), the slots hold 1.5 bytes per pixel on
the device and pinned, and the callback does no per-pixel work.  `yuv420_planes` splits such frames into their planes.
"""
from __future__ import annotations

from collections import deque
from typing import Callable, Deque, List, Optional

import torch

from . import hip_ops as ops
from .vae import HipWanVAEDecoder

PIXEL_FORMATS = {"rgb24": None, "yuv420p": "i420", "nv12": "nv12"}       # -> the layout of hip_ops.frames_yuv420


def yuv420_planes(frames: torch.Tensor, layout: str = "i420"):
    """`frames` uint8 `[..., H * 3 / 2, W]` (one frame, a block, a video; the last two dimensions contiguous) -> `(Y, U, V)` as views:
    `Y` `[..., H, W]`, `U` and `V` `[..., H / 2, W / 2]`.  `layout` "i420" (alias "yuv420p") or "nv12"; for `nv12` U and V are strided
    views of the interleaved plane."""
    layout = PIXEL_FORMATS.get(layout) or layout
    if layout not in ops.YUV420_LAYOUTS:
        raise ValueError(f"yuv420_planes: layout is one of {sorted(ops.YUV420_LAYOUTS)}, got {layout!r}")
    rows, W = frames.shape[-2:]
    H = rows * 2 // 3
    if rows % 3 or H % 2 or W % 2:
        raise ValueError(f"yuv420_planes: [{rows}, {W}] is not H * 3 / 2 rows of an even H x W frame")
    lead = tuple(frames.shape[:-2])
    flat = frames.view(*lead, rows * W)
    y = flat[..., :H * W].view(*lead, H, W)
    if layout == "i420":
        q = H * W // 4
        return y, flat[..., H * W:H * W + q].view(*lead, H // 2, W // 2), flat[..., H * W + q:].view(*lead, H // 2, W // 2)
    uv = flat[..., H * W:].view(*lead, H // 2, W // 2, 2)
    return y, uv[..., 0], uv[..., 1]


class _Slot:
    """One block in flight: the device frames, their pinned host copy and the two events."""

    def __init__(self):
        self.dev: Optional[torch.Tensor] = None          # uint8 [capacity] on the device
        self.host: Optional[torch.Tensor] = None         # uint8 [capacity] pinned
        self.views: List[torch.Tensor] = []              # per sample: host uint8 [T, H, W, 3]
        self.decoded: Optional[torch.cuda.Event] = None
        self.copied: Optional[torch.cuda.Event] = None
        self.source = None                               # what the decode reads, kept alive while the slot is in flight


class _SlotStream:
    """What `FrameStream` and `MagiFrameStream` share: `slots` device / pinned buffers in a ring, one copy stream, delivery in push order
    with the device-error word read before a block is handed out.  A subclass's `push` takes a slot (`_take_slot`, `_reserve`), has its
    decoder fill `slot.dev`, and hands the slot to `_send`."""

    _what = "FrameStream"

    def __init__(self, device, num_samples: int, slots: int, callback, keep: bool, timing: bool, pixel_format: str = "rgb24",
                 matrix: str = "bt601", full_range: bool = False):
        if pixel_format not in PIXEL_FORMATS:
            raise ValueError(f"{self._what}: pixel_format is one of {sorted(PIXEL_FORMATS)}, got {pixel_format!r}")
        if (matrix, bool(full_range)) not in ops.YUV420_PRESETS:
            raise ValueError(f"{self._what}: matrix is one of {sorted({m for m, _ in ops.YUV420_PRESETS})}, got {matrix!r}")
        self.pixel_format, self.matrix, self.full_range = pixel_format, matrix, bool(full_range)
        self._yuv = None if pixel_format == "rgb24" else dict(layout=PIXEL_FORMATS[pixel_format], matrix=matrix,
                                                              full_range=bool(full_range))
        self.num_samples, self.callback, self.keep = num_samples, callback, keep
        self.device = device
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._slots = [_Slot() for _ in range(slots)]
        self._inflight: Deque[_Slot] = deque()                     # push order; at most `slots`
        self._next = 0
        self._kept: List[List[torch.Tensor]] = [[] for _ in range(num_samples)]
        self._timing = timing
        self.events: List[tuple] = []
        self.frames_pushed = 0                                     # video frames per sample since construction / reset()

    # ---- producer side --------------------------------------------------------------------------------------------------
    def _take_slot(self) -> _Slot:
        if len(self._inflight) == len(self._slots):                # every buffer in flight: wait for the oldest (= the next slot)
            self._deliver(self._inflight.popleft(), wait=True)
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        return slot

    def _block(self, T: int, H: int, W: int):
        """(shape, bytes) of one sample's block of `T` frames of `H` x `W` in the stream's pixel format."""
        if self._yuv is None:
            return (T, H, W, 3), T * H * W * 3
        if H % 2 or W % 2:
            raise ValueError(f"{self._what}: pixel_format {self.pixel_format!r} needs an even frame size, got {H} x {W}")
        return (T, H * 3 // 2, W), T * H * W * 3 // 2

    def _reserve(self, slot: _Slot, cap: int) -> None:
        if slot.dev is None or slot.dev.numel() < cap:
            slot.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            slot.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)

    def _send(self, slot: _Slot, shape, per: int) -> None:
        """The decode of `num_samples` blocks of `shape` (`per` bytes each) into `slot.dev` is enqueued on the current stream: record
        `decoded` there, start the copy behind it, deliver whatever has arrived."""
        B = self.num_samples
        slot.decoded = torch.cuda.Event(enable_timing=self._timing)
        slot.copied = torch.cuda.Event(enable_timing=self._timing)
        slot.decoded.record()
        self._copy_stream.wait_event(slot.decoded)
        with torch.cuda.stream(self._copy_stream):
            slot.host[:B * per].copy_(slot.dev[:B * per], non_blocking=True)
            slot.copied.record()
        slot.views = [slot.host[s * per:(s + 1) * per].view(shape) for s in range(B)]
        if self._timing:
            self.events.append((slot.decoded, slot.copied))
        self._inflight.append(slot)
        self.frames_pushed += shape[0]

    # ---- consumer side --------------------------------------------------------------------------------------------------
    def poll(self) -> int:
        """Deliver every block whose copy has completed, in push order, sample by sample; -> blocks delivered.  Never waits."""
        n = 0
        while self._inflight and self._inflight[0].copied.query():
            self._deliver(self._inflight.popleft())
            n += 1
        return n

    def flush(self) -> None:
        """Wait for everything pushed so far and deliver it."""
        while self._inflight:
            self._deliver(self._inflight.popleft(), wait=True)

    def _deliver(self, slot: _Slot, wait: bool = False) -> None:
        if wait:
            slot.copied.synchronize()
        slot.source = None                                         # the copy has completed, so has the decode in front of it
        try:
            ops.check_device(f"{self._what} (block not delivered)")
        except Exception:
            self._quiesce()                                        # nothing later is delivered; let the copies in flight land first
            for s in self._inflight:
                s.source = None
            self._inflight.clear()
            raise
        for s, frames in enumerate(slot.views):
            if self.keep:
                self._kept[s].append(torch.empty(frames.shape, dtype=torch.uint8).copy_(frames))
            if self.callback is not None:
                self.callback(frames)

    def _quiesce(self) -> None:
        self._copy_stream.synchronize()

    def video(self) -> Optional[torch.Tensor]:
        """`keep=True`: every frame delivered since construction / `reset()`, host uint8 `[B, T, H, W, 3]` (`[B, T, H * 3 / 2, W]` in
        a YUV pixel format; None before the first)."""
        self.flush()
        if not self.keep or not self._kept[0]:
            return None
        return torch.stack([torch.cat(k, dim=0) for k in self._kept], dim=0)


class FrameStream(_SlotStream):
    """`push(block_latent)` per generated block, `callback(frames)` per sample per block with `frames` a host uint8 `[T, H, W, 3]`
    tensor, in push order.

    `frames` is a view of one of `slots` pinned buffers: it stays valid until `slots` further pushes have been made (the callback
    copies what it wants to keep longer).  `keep=True` keeps an unpinned host copy of every block for `video()`.  Before a block is
    delivered its copy has completed, and the device-error word is read at that point (`hip_ops.check_device`): a kernel that gave up a
    device-side wait raises there, and neither that block nor any later one is delivered.  `timing=True` records timed events and
    keeps `(decoded, copied)` per push in `events` (tools/bench_stream.py)."""

    def __init__(self, vae, num_samples: int = 1, slots: int = 3, callback: Optional[Callable[[torch.Tensor], None]] = None,
                 keep: bool = False, timing: bool = False, pixel_format: str = "rgb24", matrix: str = "bt601",
                 full_range: bool = False):
        model = getattr(vae, "model", None)
        if not isinstance(model, HipWanVAEDecoder):
            raise TypeError(f"continuous streaming needs the HIP decoder: vae.model must be a HipWanVAEDecoder "
                            f"(inferix_amd.vae.HipWanVAEWrapper), got {type(model).__name__ if model is not None else type(vae).__name__}")
        if num_samples < 1 or slots < 1:
            raise ValueError(f"FrameStream: num_samples ({num_samples}) and slots ({slots}) must be positive")
        self._decoders = [model.fork() for _ in range(num_samples)]
        super().__init__(model.device, num_samples, slots, callback, keep, timing, pixel_format, matrix, full_range)

    @torch.no_grad()
    def push(self, block_latent: torch.Tensor) -> None:
        """`block_latent` `[B, nf, C, h, w]`: decode it on the current stream as the continuation of every sample's stream, start the
        copy to the host, deliver whatever has arrived."""
        B, nf, _, h, w = block_latent.shape
        assert B == self.num_samples, f"FrameStream for {self.num_samples} samples got a block of {B}"
        slot = self._take_slot()
        H, W = 8 * h, 8 * w
        t_out = 4 * nf if self._decoders[0]._started else 4 * nf - 3
        shape, per = self._block(t_out, H, W)
        self._reserve(slot, B * self._block(4 * nf, H, W)[1])      # sized for a later block, so that the opening one does not regrow
        zs = block_latent.permute(0, 2, 1, 3, 4)
        for s, dec in enumerate(self._decoders):
            out = slot.dev[s * per:(s + 1) * per].view(shape)
            if self._yuv is None:
                dec.cached_decode_u8(zs[s:s + 1], out=out)
            else:
                dec.cached_decode_yuv420(zs[s:s + 1], out=out, **self._yuv)
        self._send(slot, shape, per)
        self.poll()

    def reset(self) -> None:
        """Deliver what is in flight, then restart every sample's stream (the next push opens a new one) and drop the kept copies."""
        self.flush()
        for dec in self._decoders:
            dec.clear_cache()
        self._kept = [[] for _ in range(self.num_samples)]
        self.frames_pushed = 0


class MagiFrameStream(_SlotStream):
    """`push(chunk)` per chunk a MAGI request hands out (`generate_per_chunk` / `ChunkSchedule.walk`), `callback(frames)` per chunk with
    `frames` a host uint8 `[T', H', W', 3]` view of one of `slots` pinned buffers, valid for `slots` further pushes, in push order.
    `keep`, `video()` (`[1, T, H, W, 3]`), `frames_pushed`, `timing` and the device-error check before a delivery are `FrameStream`'s.

    A chunk is decoded as `post_chunk_process` decodes it (`1 / scale_factor`, tiles of 256 x 256 at overlap 0.25, temporal tiles of
    `fps // 2`); the tile blend writes the channel-last uint8 frames straight into the slot's device buffer (ifx_vit_tile_blend_hwc: no
    transposing pass, no second device buffer).  The decode runs on a stream of its own (measured against a decode on the denoising
    stream: profiles/r23_magi_streaming.md):

        denoising stream:  ... integrate (the hand-out)   event `ready`     next forward ...
        decode stream:     wait(ready); chunk / scale_factor, tile forwards, blend -> uint8 [T', H', W', 3]   event `decoded`
        copy stream:       wait(decoded); uint8 device -> pinned host, asynchronous                            event `copied`

    The denoising stream waits for neither, and `push` does not synchronise the host unless every slot is in flight.  What that asks:

      * the chunk is a view of the request's clip, which later steps never write; the slot holds the view (and with it the clip) until
        its copy, and so its decode, has completed: the caching allocator cannot hand the clip out again under a running decode;
      * the VAE's cached arenas, tables and scratch belong to this stream from its first push until `flush()`: nothing else may decode
        with the same `vae` object in between.  `flush()` and `reset()` synchronise the decode stream before they return, after which
        the same `vae` can be used on the current stream again (`run_text_to_video` behind a streamed call);
      * two side streams in all (decode, copy); the process's hardware-queue setting is left alone.

    The chunks of a request are independent decodes (`temporal_tile_overlap_factor` 0, as upstream), so nothing is carried from one push
    to the next and `reset()` only drops the kept copies.

    In a YUV `pixel_format` the blend writes its `rgb24` frames into a device scratch buffer of the stream's — one per chunk shape met
    since the last `reset()`, which drops them — and `ifx_rgb8_yuv420` converts into the slot behind it on the decode stream."""

    _what = "MagiFrameStream"

    def __init__(self, vae, config, slots: int = 3, callback: Optional[Callable[[torch.Tensor], None]] = None, keep: bool = False,
                 timing: bool = False, pixel_format: str = "rgb24", matrix: str = "bt601", full_range: bool = False):
        from .magi.vae import HipMagiVAEDecoder
        if not isinstance(vae, HipMagiVAEDecoder):
            raise TypeError(f"continuous streaming needs the HIP decoder: vae must be a HipMagiVAEDecoder (inferix_amd.magi.vae), "
                            f"got {type(vae).__name__}")
        if slots < 1:
            raise ValueError(f"MagiFrameStream: slots ({slots}) must be positive")
        self.vae, self.config = vae, config
        self._shapes = {}                                          # (f, h, w) of a chunk -> (T', H', W', 3) of its frames
        self._rgb = {}                                             # YUV formats: frame shape -> the blend's uint8 [T', H', W', 3] scratch
        super().__init__(torch.device(vae.decoder.device), 1, slots, callback, keep, timing, pixel_format, matrix, full_range)
        self._decode_stream = torch.cuda.Stream(device=self.device)

    def _quiesce(self) -> None:
        self._decode_stream.synchronize()
        self._copy_stream.synchronize()

    def flush(self) -> None:
        """Wait for everything pushed so far and deliver it; the decode stream is idle afterwards (the `vae` is the caller's again)."""
        try:
            super().flush()
        finally:
            self._decode_stream.synchronize()

    @torch.no_grad()
    def push(self, chunk: torch.Tensor) -> None:
        """`chunk` `[1, C, f, h, w]`, the view `walk` yields (later steps never write it): start its decode behind the hand-out, the
        copy to the host behind the decode, deliver whatever has arrived."""
        from .magi.vae import decode_chunk
        N, _, f, h, w = chunk.shape
        assert N == 1, f"MagiFrameStream streams one sample, got a chunk of {N}"
        rc = self.config.runtime_config
        shape = self._shapes.get((f, h, w))
        if shape is None:                                          # what the tiles of this chunk decode to (a single-frame tile: one frame)
            plan = self.vae.tile_plan((f, h, w), 256, 256, rc.fps // 2, 0.25, 0, True)
            shape = self._shapes[(f, h, w)] = tuple(plan.out_shape) + (3,)
        out_shape, per = self._block(*shape[:3])
        slot = self._take_slot()
        self._reserve(slot, per)
        ds = self._decode_stream
        ready = torch.cuda.Event()
        ready.record()                                             # behind the hand-out on the denoising stream
        slot.source = chunk                                        # the clip stays alive until the slot's decode has completed
        slot.dev.record_stream(ds)
        rgb = None
        if self._yuv is not None:                                  # the blend keeps writing rgb24, into a scratch of this stream's
            rgb = self._rgb.get(shape)
            if rgb is None:
                rgb = self._rgb[shape] = torch.empty(shape, dtype=torch.uint8, device=self.device)
                rgb.record_stream(ds)
        ds.wait_event(ready)
        with torch.cuda.stream(ds):
            if rgb is None:
                decode_chunk(chunk, self.vae, rc.scale_factor, rc.fps // 2, uint8_output=slot.dev[:per].view(1, *shape))
            else:                                                  # one more pass of 4.5 bytes per pixel on the decode stream, behind the blend
                decode_chunk(chunk, self.vae, rc.scale_factor, rc.fps // 2, uint8_output=rgb.view(1, *shape))
                ops.rgb8_to_yuv420(rgb, out=slot.dev[:per].view(out_shape), **self._yuv)
            self._send(slot, out_shape, per)
        self.poll()

    def reset(self) -> None:
        """Deliver what is in flight and drop the kept copies and, in a YUV format, the rgb24 scratch buffers (one per chunk shape seen
        since the last `reset()`; `flush()` has synchronised the decode stream, their only user)."""
        self.flush()
        self._rgb.clear()
        self._kept = [[]]
        self.frames_pushed = 0

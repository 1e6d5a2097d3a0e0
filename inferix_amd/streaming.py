"""`FrameStream`: one continuous VAE stream per sample, uint8 frames finished on the device, handed to the consumer without stalling
the denoising loop.

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
"""
from __future__ import annotations

from collections import deque
from typing import Callable, Deque, List, Optional

import torch

from . import hip_ops as ops
from .vae import HipWanVAEDecoder


class _Slot:
    """One block in flight: the device frames, their pinned host copy and the two events."""

    def __init__(self):
        self.dev: Optional[torch.Tensor] = None          # uint8 [capacity] on the device
        self.host: Optional[torch.Tensor] = None         # uint8 [capacity] pinned
        self.views: List[torch.Tensor] = []              # per sample: host uint8 [T, H, W, 3]
        self.decoded: Optional[torch.cuda.Event] = None
        self.copied: Optional[torch.cuda.Event] = None


class FrameStream:
    """`push(block_latent)` per generated block, `callback(frames)` per sample per block with `frames` a host uint8 `[T, H, W, 3]`
    tensor, in push order.

    `frames` is a view of one of `slots` pinned buffers: it stays valid until `slots` further pushes have been made (the callback
    copies what it wants to keep longer).  `keep=True` keeps an unpinned host copy of every block for `video()`.  Before a block is
    delivered its copy has completed, and the device-error word is read at that point (`hip_ops.check_device`): a kernel that gave up a
    device-side wait raises there, and neither that block nor any later one is delivered.  `timing=True` records timed events and
    keeps `(decoded, copied)` per push in `events` (tools/bench_stream.py)."""

    def __init__(self, vae, num_samples: int = 1, slots: int = 3, callback: Optional[Callable[[torch.Tensor], None]] = None,
                 keep: bool = False, timing: bool = False):
        model = getattr(vae, "model", None)
        if not isinstance(model, HipWanVAEDecoder):
            raise TypeError(f"continuous streaming needs the HIP decoder: vae.model must be a HipWanVAEDecoder "
                            f"(inferix_amd.vae.HipWanVAEWrapper), got {type(model).__name__ if model is not None else type(vae).__name__}")
        if num_samples < 1 or slots < 1:
            raise ValueError(f"FrameStream: num_samples ({num_samples}) and slots ({slots}) must be positive")
        self.num_samples, self.callback, self.keep = num_samples, callback, keep
        self.device = model.device
        self._decoders = [model.fork() for _ in range(num_samples)]
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._slots = [_Slot() for _ in range(slots)]
        self._inflight: Deque[_Slot] = deque()                     # push order; at most `slots`
        self._next = 0
        self._kept: List[List[torch.Tensor]] = [[] for _ in range(num_samples)]
        self._timing = timing
        self.events: List[tuple] = []
        self.frames_pushed = 0                                     # video frames per sample since construction / reset()

    # ---- producer side --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def push(self, block_latent: torch.Tensor) -> None:
        """`block_latent` `[B, nf, C, h, w]`: decode it on the current stream as the continuation of every sample's stream, start the
        copy to the host, deliver whatever has arrived."""
        B, nf, _, h, w = block_latent.shape
        assert B == self.num_samples, f"FrameStream for {self.num_samples} samples got a block of {B}"
        if len(self._inflight) == len(self._slots):                # every buffer in flight: wait for the oldest (= the next slot)
            self._deliver(self._inflight.popleft(), wait=True)
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        H, W = 8 * h, 8 * w
        t_out = 4 * nf if self._decoders[0]._started else 4 * nf - 3
        per, cap = t_out * H * W * 3, B * 4 * nf * H * W * 3       # sized for a later block, so that the opening one does not regrow
        if slot.dev is None or slot.dev.numel() < cap:
            slot.dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            slot.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        zs = block_latent.permute(0, 2, 1, 3, 4)
        for s, dec in enumerate(self._decoders):
            dec.cached_decode_u8(zs[s:s + 1], out=slot.dev[s * per:(s + 1) * per].view(t_out, H, W, 3))
        slot.decoded = torch.cuda.Event(enable_timing=self._timing)
        slot.copied = torch.cuda.Event(enable_timing=self._timing)
        slot.decoded.record()
        self._copy_stream.wait_event(slot.decoded)
        with torch.cuda.stream(self._copy_stream):
            slot.host[:B * per].copy_(slot.dev[:B * per], non_blocking=True)
            slot.copied.record()
        slot.views = [slot.host[s * per:(s + 1) * per].view(t_out, H, W, 3) for s in range(B)]
        if self._timing:
            self.events.append((slot.decoded, slot.copied))
        self._inflight.append(slot)
        self.frames_pushed += t_out
        self.poll()

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
        try:
            ops.check_device("FrameStream (block not delivered)")
        except Exception:
            self._copy_stream.synchronize()                        # nothing later is delivered; let the copies in flight land first
            self._inflight.clear()
            raise
        for s, frames in enumerate(slot.views):
            if self.keep:
                self._kept[s].append(torch.empty(frames.shape, dtype=torch.uint8).copy_(frames))
            if self.callback is not None:
                self.callback(frames)

    def reset(self) -> None:
        """Deliver what is in flight, then restart every sample's stream (the next push opens a new one) and drop the kept copies."""
        self.flush()
        for dec in self._decoders:
            dec.clear_cache()
        self._kept = [[] for _ in range(self.num_samples)]
        self.frames_pushed = 0

    def video(self) -> Optional[torch.Tensor]:
        """`keep=True`: every frame delivered since construction / `reset()`, host uint8 `[B, T, H, W, 3]` (None before the first)."""
        self.flush()
        if not self.keep or not self._kept[0]:
            return None
        return torch.stack([torch.cat(k, dim=0) for k in self._kept], dim=0)

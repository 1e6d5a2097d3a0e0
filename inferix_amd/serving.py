"""SessionBatch — several independent Self-Forcing sessions served from one process, one block at a time.

A batch of `CausalInferencePipeline.inference` shares ONE position: every row starts together and ends together.  Viewers do not
arrive together.  Here every session owns its cache request, its per-layer cache meta, its text embedding, its noise generator, its
block counter and its frame stream, and one `step()` advances every live session by one block with RAGGED generator forwards: the
rows of a forward are at different positions of their videos (`HipCausalWanModel.forward` with per-sample `current_start` / meta
lists; the samples' self-attention in one launch, `ifx_attn_fwd_multi`).  A session opened between two steps joins at the next one,
at ITS block 0, and projects its text K / V there while its neighbours reuse theirs.

    sb = SessionBatch(pipe, max_sessions=8)          # pipe: SelfForcingPipeline on a few-step config (denoising_step_list)
    a = sb.open("prompt A", seed=1, stream_callback=cb, continuous=True, pixel_format="nv12")
    sb.step()                                        # {session: latents [1, nf, C, H, W]} of the block every live session made
    b = sb.open("prompt B", seed=2)                  # joins at the next step
    sb.step(); sb.close(a); sb.run(num_blocks=5)

What a step does is the block body of `CausalInferencePipeline.inference`: the denoising steps of `denoising_step_list` with ONE
`add_noise` over all rows in between, then the clean-context re-run; the timestep is the same for every row.  The noise of a session
is drawn from that session's own `torch.Generator`, so it does not depend on who else is live.  There is no host synchronisation
inside a step beyond what `FrameStream.poll` does.

Not built in `SessionBatch` (refused with the reason at construction or `open`): many-step configs, `world_size > 1`,
`independent_first_frame`, `initial_latent` / I2V, more than `max_sessions` sessions.

`InteractiveSessionBatch(SessionBatch)` (below) lifts three of those and the block-boundary join: its sessions move one forward at a
time (`advance()`), so a forward's rows may be in different phases of their blocks — per-row timesteps — and a session may start from
given frames (`open(initial_latent=)` / `open(image=)`), run on an `independent_first_frame` config, change its prompt at its next block
boundary (`set_prompt`) and join at the next forward instead of the next block.  Its docstring holds the work items, the order of a
session's noise draws and what a prompt change does.

Out of scope for both: recomputing a live cache under a new prompt without the restart, CausVid, MAGI and many-step configs,
`world_size > 1`, consumer threads, mixed resolutions in one batch."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from .kvcache_manager import KVCacheManager, KVCacheRequest


class Session:
    """One viewer's state.  Handed out by `SessionBatch.open`; the fields are read-only for the caller."""

    def __init__(self, index: int, prompt: str, seed: int):
        self.index, self.prompt, self.seed = index, prompt, seed
        self.block = 0                      # blocks made so far
        self.frames_done = 0                # latent frames made so far (the position of the next block)
        self.position = 0                   # InteractiveSessionBatch: the next block's frame in the cache (0 again after a prompt change)
        self.segment = 0                    # prompt changes that have taken effect
        self.forwards = 0                   # generator forwards the session took part in
        self.request: Optional[KVCacheRequest] = None
        self.kv_meta: List[dict] = []
        self.cross_meta: List[dict] = []
        self.prompt_embeds: Optional[torch.Tensor] = None
        self.generator: Optional[torch.Generator] = None
        self.stream = None                  # FrameStream(num_samples=1) of a continuous=True session
        self.closed = False
        self._queue: list = []              # InteractiveSessionBatch: the work items in front of the session, head first
        self._x = self._x0 = self._keep = self._pending = None

    @property
    def phase(self):
        """`(kind, step index)` of the session's next forward — `("PREFILL", None)`, `("DENOISE", i)`, `("RERUN", None)` — or None
        between two blocks."""
        return (self._queue[0].kind, self._queue[0].index) if self._queue else None

    def __repr__(self):
        return f"Session({self.index}, block={self.block}{', closed' if self.closed else ''})"


class SessionBatch:
    _independent_first_frame = False    # whether 1-frame opening blocks are built (InteractiveSessionBatch)

    def __init__(self, pipe, max_sessions: int = 8):
        inner = getattr(pipe, "pipeline", None)
        if getattr(pipe, "_pipeline_type", None) != "causal" or not hasattr(getattr(inner, "args", None), "denoising_step_list"):
            raise NotImplementedError("SessionBatch is built for the few-step pipeline (configs with denoising_step_list); this config "
                                      "selects the many-step CausalDiffusionInferencePipeline")
        if getattr(pipe.parallel_config, "world_size", 1) > 1:
            raise NotImplementedError(f"SessionBatch runs on one GPU: world_size {pipe.parallel_config.world_size} (ragged forwards "
                                      "are not built for sequence parallelism)")
        if getattr(inner, "independent_first_frame", False) and not self._independent_first_frame:
            raise NotImplementedError("SessionBatch: independent_first_frame configs are not built (every block of every session has "
                                      "num_frame_per_block frames)")
        if max_sessions < 1:
            raise ValueError(f"SessionBatch: max_sessions must be positive, got {max_sessions}")
        if inner.text_encoder is None:
            raise RuntimeError("SessionBatch needs a text_encoder: pass text_encoder=... to SelfForcingPipeline")
        self.pipe, self.inner, self.max_sessions = pipe, inner, int(max_sessions)
        self.device = torch.device(pipe.device)
        self.kvm = KVCacheManager(device=self.device)
        self.sessions: List[Session] = []          # live, in the order they were opened (= row order of a forward)
        self._opened = 0
        self.dtype = torch.bfloat16

    # ---- sessions -----------------------------------------------------------------------------------------------------
    def open(self, prompt: str, seed: int = 0, stream_callback: Optional[Callable[[torch.Tensor], None]] = None,
             continuous: bool = False, keep_video: bool = False, pixel_format: str = "rgb24", color_matrix: str = "bt601",
             full_range: bool = False, initial_latent: Optional[torch.Tensor] = None) -> Session:
        """A new session; it makes its block 0 at the next `step()`.  `continuous=True` gives it a `FrameStream` of its own (formats and
        keywords of `run_streaming_generation`): `stream_callback(frames)` per block, `keep_video=True` keeps the frames for
        `session.stream.video()`."""
        if initial_latent is not None:
            raise NotImplementedError("SessionBatch.open: initial_latent (image-to-video, segment overlap) is not built for sessions")
        if len(self.sessions) >= self.max_sessions:
            raise RuntimeError(f"SessionBatch.open: {len(self.sessions)} sessions are live and max_sessions is {self.max_sessions}; "
                               "close one first")
        if not continuous and (stream_callback is not None or pixel_format != "rgb24"):
            raise ValueError("SessionBatch.open: frames are streamed by a session's own FrameStream only: stream_callback / pixel_format "
                             "need continuous=True")
        inner = self.inner
        s = Session(self._opened, prompt, int(seed))
        if continuous:
            from .streaming import FrameStream
            if inner.vae is None:
                raise RuntimeError("SessionBatch.open: continuous=True needs a vae: pass vae=... to SelfForcingPipeline")
            try:
                s.stream = FrameStream(inner.vae, num_samples=1, callback=stream_callback, keep=keep_video, pixel_format=pixel_format,
                                       matrix=color_matrix, full_range=full_range)
            except TypeError as exc:
                raise ValueError(f"continuous=True: {exc}") from exc
        s.request = KVCacheRequest(f"session_{s.index}")
        size = inner.local_attn_size * inner.frame_seq_length if inner.local_attn_size != -1 \
            else getattr(inner.args, "kv_cache_tokens", 32760)
        inner._walk_caches("allocate_kv_cache", [self.kvm], [s.request], sequence_length=size, dtype=self.dtype, ulysses_size=1,
                           ring_size=1)
        inner._walk_caches("allocate_crossattn_cache", [self.kvm], [s.request],
                           crossattn_length=getattr(inner.generator.model, "text_len", 512), dtype=self.dtype)
        s.kv_meta = inner._fresh_kv_meta(inner.num_transformer_blocks)
        s.cross_meta = inner._fresh_crossattn_meta(inner.num_transformer_blocks)
        embeds = inner.text_encoder(text_prompts=[prompt])["prompt_embeds"]
        s.prompt_embeds = embeds[0]
        s.generator = torch.Generator(device=self.device).manual_seed(s.seed)
        self._opened += 1
        self.sessions.append(s)
        return s

    def close(self, session: Session) -> None:
        """Deliver what the session's stream still holds, free its caches, take it out of the batch."""
        if session.closed:
            return
        session.closed = True
        self.sessions.remove(session)
        try:
            if session.stream is not None:
                session.stream.flush()
        finally:
            self.inner._walk_caches("clear_cache", [self.kvm], [session.request])
            if session.request.request_id in getattr(self.kvm, "request_to_kv_caches", {}):
                self.kvm.free(session.request)
            session.kv_meta, session.cross_meta, session.prompt_embeds = [], [], None
            session._queue = []
            session._x = session._x0 = session._keep = session._pending = None

    def close_all(self) -> None:
        for s in list(self.sessions):
            self.close(s)

    # ---- one block of every live session ------------------------------------------------------------------------------
    def _draw(self, nf: int) -> torch.Tensor:
        """Gaussian `[B, nf, C, H, W]`: row i from session i's own generator."""
        shape = [1, nf, *self.pipe.latent_shape]
        return torch.cat([torch.randn(shape, generator=s.generator, device=self.device, dtype=self.dtype) for s in self.sessions])

    @torch.no_grad()
    def step(self) -> Dict[Session, torch.Tensor]:
        """Every live session advances ONE block -> `{session: latents [1, nf, C, H, W]}` (views of one tensor; the block has been
        pushed into the session's stream, its frames arrive through the callback)."""
        live = list(self.sessions)
        if not live:
            return {}
        inner, dev = self.inner, self.device
        B, nf = len(live), inner.num_frame_per_block
        fsl = inner.frame_seq_length
        cond = {"prompt_embeds": [s.prompt_embeds for s in live]}
        reqs = [s.request for s in live]
        if B == 1:        # a lone session: the uniform call, exactly as CausalInferencePipeline makes it
            where = dict(kv_cache_meta=live[0].kv_meta, crossattn_cache_meta=live[0].cross_meta, current_start=live[0].frames_done * fsl)
        else:
            where = dict(kv_cache_meta=[s.kv_meta for s in live], crossattn_cache_meta=[s.cross_meta for s in live],
                         current_start=[s.frames_done * fsl for s in live])

        def gen(x, timestep):
            return inner.generator(noisy_image_or_video=x, conditional_dict=cond, timestep=timestep, kv_cache_manager=self.kvm,
                                   kv_cache_requests=reqs, **where)
        x = self._draw(nf)
        steps = inner.denoising_step_list
        x0 = timestep = None
        for index, tcur in enumerate(steps):
            timestep = inner._timestep(tcur, (B, nf), dev)
            _, x0 = gen(x, timestep)
            if index < len(steps) - 1:
                flat = x0.flatten(0, 1)
                eps = self._draw(nf).flatten(0, 1).to(flat.dtype)
                tn = inner._timestep(steps[index + 1], (B * nf,), dev, torch.long)
                x = inner.scheduler.add_noise(flat, eps, tn).unflatten(0, x0.shape[:2])
        ctx_t = inner._timestep(getattr(inner.args, "context_noise", 0), tuple(timestep.shape), dev, timestep.dtype)
        gen(x0, ctx_t)                                   # clean-context re-run: the block's K / V rows as later blocks read them
        out = {}
        for i, s in enumerate(live):
            s.block += 1
            s.frames_done += nf
            s.position = s.frames_done
            s.forwards += len(steps) + 1
            out[s] = x0[i:i + 1]
            if s.stream is not None:
                s.stream.push(out[s])
        return out

    def run(self, num_blocks: int) -> Dict[Session, torch.Tensor]:
        """`num_blocks` steps -> `{session: latents [1, num_blocks * nf, C, H, W]}` for the sessions live throughout."""
        blocks: Dict[Session, List[torch.Tensor]] = {}
        for _ in range(num_blocks):
            for s, lat in self.step().items():
                blocks.setdefault(s, []).append(lat.clone())
        return {s: torch.cat(b, dim=1) for s, b in blocks.items() if len(b) == num_blocks}


PREFILL, DENOISE, RERUN = "PREFILL", "DENOISE", "RERUN"


class _Item:
    """One generator forward over `n` frames of one session.  PREFILL: `latents` are the input rows, `given` says they are new frames
    of the viewer's video (counted, streamed, retained) and not a prompt change's overlap.  DENOISE: `index` is the denoising step."""
    __slots__ = ("kind", "n", "index", "latents", "given")

    def __init__(self, kind: str, n: int, index: Optional[int] = None, latents: Optional[torch.Tensor] = None, given: bool = False):
        self.kind, self.n, self.index, self.latents, self.given = kind, n, index, latents, given


class InteractiveSessionBatch(SessionBatch):
    """`SessionBatch` whose sessions move one generator FORWARD at a time, so that they need not be in the same phase of a block:

        sb = InteractiveSessionBatch(pipe, max_sessions=8, keep_frames=3)
        a = sb.open("prompt A", seed=1, continuous=True, stream_callback=cb)
        sb.advance(); sb.advance()                       # two forwards of a's block 0
        b = sb.open("prompt B", seed=2, image=first_frame)   # in the NEXT forward: its prefill at t = 0 beside a's third denoising step
        sb.set_prompt(a, "prompt A, at night")           # falls due when a's block in flight is done
        sb.step()                                        # forwards until a and b have each finished one more block

    Every session holds a queue of work items, one per forward:

        PREFILL    given latents [pos, pos + n) at timestep 0 (the `t0` of `inference`)       -> position += n
        DENOISE i  noise (i = 0) or the re-noised x0, at `denoising_step_list[i]`             -> i < S - 1: re-noise to step i + 1; else keep x0
        RERUN      x0 at `args.context_noise`                                                 -> block done: position += n, block += 1, streamed

    `advance()` takes the head item of every live session (a session between two blocks plans its next block first), groups the sessions
    by the frame count of that item (at most two groups: 1 and `num_frame_per_block`), runs ONE generator forward per group — ragged in
    position AND in timestep: `[B, n]` with a row's own value — and applies every row's post-step; it returns the sessions whose block
    finished.  `step()` calls `advance()` until every session live on entry has finished exactly one more block (a session that is done
    sits out the rest), which without given frames, prompt changes or `advance()` calls is forward for forward `SessionBatch.step`: same
    rows, order, tagged timestep constants and noise draws.

    The block plan is `BlockLoopPipeline._block_plan` / `_prefill` per session: blocks of `num_frame_per_block` frames; on an
    `independent_first_frame` config a session without given frames opens with a 1-frame block; given frames (`open(initial_latent=)` or
    `open(image=)`, encoded as `run_image_to_video` does) are prefilled block by block — on an `independent_first_frame` config the
    first frame alone, so there must be `1 + k * num_frame_per_block` of them, otherwise a multiple of `num_frame_per_block`.  They are
    the start of the viewer's video: counted in `frames_done`, pushed into a `continuous=True` session's stream (one push per prefill
    item) before its first generated block, never returned by `step()` / `advance()`.

    `set_prompt(session, prompt, overlap_frames=None)` is a segment boundary of `run_interactive_generation` for ONE session: at the
    session's next block boundary its prompt is encoded, its cache meta reset (the caches are reused: rows past `local_end` are never
    read), its position set to 0 and the last `overlap_frames` clean latents of its video (the batch retains `keep_frames` per session,
    given frames included) are prefilled under the new prompt.  `segment` counts up, `block`, `frames_done` and the generator state
    carry on, the overlap is not streamed again and the decoder stream is not reset: the viewer's video has no seam.

    THE DRAWS of a session's own `torch.Generator(device).manual_seed(seed)`, a contract: per generated block one `[1, n, C, H, W]` bf16
    noise tensor, then S - 1 eps tensors of that shape in step order (S = `len(denoising_step_list)`).  PREFILL and RERUN draw nothing,
    `set_prompt` does not reseed, and nothing a neighbour does changes a session's draws.

    `open`, `set_prompt`, `close`, `advance` and `step` are called from one thread.  Out of scope: recomputing a live cache under a new
    prompt without the restart; CausVid, MAGI and many-step configs; `world_size > 1`; consumer threads; mixed resolutions in one
    batch."""
    _independent_first_frame = True

    def __init__(self, pipe, max_sessions: int = 8, keep_frames: Optional[int] = None):
        super().__init__(pipe, max_sessions)
        keep = self.inner.num_frame_per_block if keep_frames is None else int(keep_frames)
        if keep < 0:
            raise ValueError(f"InteractiveSessionBatch: keep_frames must be non-negative, got {keep_frames}")
        self.keep_frames = keep
        self._t_rows: dict = {}             # timestep tensors of forwards whose rows hold different values, by those values

    # ---- the block plan of one session --------------------------------------------------------------------------------------
    def _prefill_sizes(self, n: int, what: str) -> List[int]:
        """The frame counts `_prefill` walks `n` given frames in; ValueError naming the rule."""
        nfb = self.inner.num_frame_per_block
        if self.inner.independent_first_frame:
            if n < 1 or (n - 1) % nfb != 0:
                raise ValueError(f"{what}: {n} frames; an independent_first_frame config takes 1 + k * num_frame_per_block "
                                 f"(1 + k * {nfb}) given frames: the first one alone, then whole blocks")
            return [1] + [nfb] * ((n - 1) // nfb)
        if n < 1 or n % nfb != 0:
            raise ValueError(f"{what}: {n} frames; given frames must be a multiple of num_frame_per_block ({nfb})")
        return [nfb] * (n // nfb)

    def _largest_valid(self, n: int) -> int:
        """The largest frame count `_prefill_sizes` takes that is at most `n` (0: none)."""
        nfb = self.inner.num_frame_per_block
        if self.inner.independent_first_frame:
            return 0 if n < 1 else 1 + (n - 1) // nfb * nfb
        return n // nfb * nfb

    def _queue_prefill(self, s: Session, latents: torch.Tensor, sizes: List[int], given: bool) -> None:
        at = 0
        for n in sizes:
            s._queue.append(_Item(PREFILL, n, latents=latents[:, at:at + n], given=given))
            at += n

    def _retain(self, s: Session, latents: torch.Tensor) -> None:
        if self.keep_frames:
            kept = latents if s._keep is None else torch.cat([s._keep, latents], dim=1)
            s._keep = kept[:, -self.keep_frames:]

    def _plan(self, s: Session) -> None:
        """A session between two blocks: a prompt change that has fallen due, then the items of its next generated block."""
        inner = self.inner
        if s._pending is not None:
            prompt, overlap = s._pending
            s._pending = None
            s.prompt = prompt
            s.prompt_embeds = inner.text_encoder(text_prompts=[prompt])["prompt_embeds"][0]
            inner._reset_kv_meta(s.kv_meta)
            inner._reset_crossattn_meta(s.cross_meta)
            s.position = 0
            s.segment += 1
            count = self._largest_valid(min(overlap, 0 if s._keep is None else s._keep.shape[1]))
            if count:
                self._queue_prefill(s, s._keep[:, -count:], self._prefill_sizes(count, "overlap"), given=False)
                return
        n = 1 if inner.independent_first_frame and s.position == 0 else inner.num_frame_per_block
        s._x = torch.randn([1, n, *self.pipe.latent_shape], generator=s.generator, device=self.device, dtype=self.dtype)
        s._queue = [_Item(DENOISE, n, i) for i in range(len(inner.denoising_step_list))] + [_Item(RERUN, n)]

    # ---- sessions ---------------------------------------------------------------------------------------------------------------
    def open(self, prompt: str, seed: int = 0, stream_callback: Optional[Callable[[torch.Tensor], None]] = None,
             continuous: bool = False, keep_video: bool = False, pixel_format: str = "rgb24", color_matrix: str = "bt601",
             full_range: bool = False, initial_latent: Optional[torch.Tensor] = None, image: Optional[torch.Tensor] = None) -> Session:
        """`SessionBatch.open`, and a session may start from given frames: `initial_latent` `[1, n, C, H, W]` (any device), or `image`
        `[1, 3, 1, H, W]` in [-1, 1], which the VAE encoder turns into one.  It takes part in the next `advance()`."""
        if initial_latent is not None and image is not None:
            raise ValueError("InteractiveSessionBatch.open: pass initial_latent or image, not both")
        if image is not None:
            vae = self.inner.vae
            if vae is None or not hasattr(vae, "encode_to_latent"):
                raise RuntimeError("InteractiveSessionBatch.open: image= needs a vae with an encoder (encode_to_latent): pass vae=... "
                                   "to SelfForcingPipeline")
            initial_latent = vae.encode_to_latent(image)
        sizes: List[int] = []
        if initial_latent is not None:
            if initial_latent.ndim != 5 or initial_latent.shape[0] != 1 or list(initial_latent.shape[2:]) != list(self.pipe.latent_shape):
                raise ValueError(f"InteractiveSessionBatch.open: initial_latent must be [1, n, {', '.join(map(str, self.pipe.latent_shape))}], "
                                 f"got {list(initial_latent.shape)}")
            sizes = self._prefill_sizes(initial_latent.shape[1], "InteractiveSessionBatch.open: initial_latent")
            initial_latent = initial_latent.to(device=self.device, dtype=self.dtype)
        s = super().open(prompt, seed, stream_callback, continuous, keep_video, pixel_format, color_matrix, full_range)
        if sizes:
            self._queue_prefill(s, initial_latent, sizes, given=True)
        return s

    def set_prompt(self, session: Session, prompt: str, overlap_frames: Optional[int] = None) -> None:
        """The session goes on under `prompt` from its next block boundary (a block in flight finishes under the old one; a second call
        before that replaces the first), restarted from the last `overlap_frames` clean latents of its video: at most `keep_frames`,
        a multiple of `num_frame_per_block` (`1 + k * num_frame_per_block` or 0 on an `independent_first_frame` config).  Left out, it
        is the largest such count within `keep_frames`.  Where the video is shorter than that, the largest count that exists is used —
        possibly none: a plain restart."""
        if session.closed:
            raise RuntimeError(f"InteractiveSessionBatch.set_prompt: {session!r} is closed")
        nfb = self.inner.num_frame_per_block
        if overlap_frames is None:
            overlap = self._largest_valid(self.keep_frames)
        else:
            overlap = int(overlap_frames)
            if overlap > self.keep_frames:
                raise ValueError(f"InteractiveSessionBatch.set_prompt: overlap_frames ({overlap}) exceeds keep_frames "
                                 f"({self.keep_frames}), the clean latents a session retains")
            if self.inner.independent_first_frame:
                if overlap < 0 or (overlap and (overlap - 1) % nfb != 0):
                    raise ValueError(f"InteractiveSessionBatch.set_prompt: overlap_frames ({overlap}) must be 0 or 1 + k * "
                                     f"num_frame_per_block (1 + k * {nfb}) on an independent_first_frame config")
            else:
                from .core.interactive import validate_overlap_config
                validate_overlap_config(overlap, nfb)
        session._pending = (prompt, overlap)

    # ---- one forward of every live session --------------------------------------------------------------------------------------
    def _timesteps(self, heads: List[_Item], n: int) -> torch.Tensor:
        """The timestep tensor of one forward, made of the pipeline's constants: no device read, no upload."""
        inner, dev, B = self.inner, self.device, len(heads)
        steps = inner.denoising_step_list
        if all(it.kind == PREFILL for it in heads):
            key = ("t0", B)
            if key not in self._t_rows:
                self._t_rows[key] = torch.zeros([B, 1], device=dev, dtype=torch.int64)       # the `t0` of `inference`
            return self._t_rows[key]
        if all(it.kind == DENOISE and it.index == heads[0].index for it in heads):
            return inner._timestep(steps[heads[0].index], (B, n), dev)
        ctx = getattr(inner.args, "context_noise", 0)
        dtype = inner._timestep(steps[-1], (B, n), dev).dtype          # what the re-run of `SessionBatch.step` takes its dtype from
        values = [steps[it.index] if it.kind == DENOISE else ctx if it.kind == RERUN else 0 for it in heads]
        scalars = tuple(float(v) for v in values)
        if all(v == scalars[0] for v in scalars):
            return inner._timestep(values[0], (B, n), dev, dtype)
        key = (scalars, n)
        if key not in self._t_rows:
            if len(self._t_rows) >= 64:
                self._t_rows.clear()
            self._t_rows[key] = torch.cat([inner._timestep(v, (1, n), dev) if it.kind == DENOISE else inner._timestep(v, (1, n), dev, dtype)
                                           for v, it in zip(values, heads)])
        return self._t_rows[key]

    def _forward(self, rows: List[Session], n: int, out: Dict[Session, torch.Tensor]) -> None:
        """One generator forward over the head items of `rows` (all of `n` frames), then every row's post-step."""
        inner, dev = self.inner, self.device
        fsl, steps = inner.frame_seq_length, inner.denoising_step_list
        heads = [s._queue.pop(0) for s in rows]
        B = len(rows)
        x = torch.cat([it.latents if it.kind == PREFILL else s._x if it.kind == DENOISE else s._x0 for s, it in zip(rows, heads)])
        if B == 1:            # a lone session: the uniform call, exactly as CausalInferencePipeline makes it
            where = dict(kv_cache_meta=rows[0].kv_meta, crossattn_cache_meta=rows[0].cross_meta, current_start=rows[0].position * fsl)
        else:
            where = dict(kv_cache_meta=[s.kv_meta for s in rows], crossattn_cache_meta=[s.cross_meta for s in rows],
                         current_start=[s.position * fsl for s in rows])
        _, x0 = inner.generator(noisy_image_or_video=x, conditional_dict={"prompt_embeds": [s.prompt_embeds for s in rows]},
                                timestep=self._timesteps(heads, n), kv_cache_manager=self.kvm,
                                kv_cache_requests=[s.request for s in rows], **where)
        again = []                                       # rows to re-noise for their next denoising step
        for i, (s, it) in enumerate(zip(rows, heads)):
            s.forwards += 1
            if it.kind == PREFILL:
                s.position += n
                if it.given:
                    s.frames_done += n
                    self._retain(s, it.latents)
                    if s.stream is not None:
                        s.stream.push(it.latents)
            elif it.kind == DENOISE:
                if it.index < len(steps) - 1:
                    again.append(i)
                else:
                    s._x0 = x0[i:i + 1]
            else:
                s.position += n
                s.frames_done += n
                s.block += 1
                self._retain(s, s._x0)
                out[s] = s._x0
                if s.stream is not None:
                    s.stream.push(s._x0)
                s._x = s._x0 = None
        if again:
            clean = x0 if len(again) == B else torch.cat([x0[i:i + 1] for i in again])
            flat = clean.flatten(0, 1)
            eps = torch.cat([torch.randn([1, n, *self.pipe.latent_shape], generator=rows[i].generator, device=dev, dtype=self.dtype)
                             for i in again]).flatten(0, 1).to(flat.dtype)
            nxt = [heads[i].index + 1 for i in again]
            if all(k == nxt[0] for k in nxt):
                tn = inner._timestep(steps[nxt[0]], (len(again) * n,), dev, torch.long)
            else:
                tn = torch.cat([inner._timestep(steps[k], (n,), dev, torch.long) for k in nxt])
            x = inner.scheduler.add_noise(flat, eps, tn).unflatten(0, clean.shape[:2])
            for j, i in enumerate(again):
                rows[i]._x = x[j:j + 1]

    def _advance(self, live: List[Session]) -> Dict[Session, torch.Tensor]:
        for s in live:
            if not s._queue:
                self._plan(s)
        groups: Dict[int, List[Session]] = {}            # by the frame count of the head item, in session order
        for s in live:
            groups.setdefault(s._queue[0].n, []).append(s)
        out: Dict[Session, torch.Tensor] = {}
        for n, rows in groups.items():
            self._forward(rows, n, out)
        return out

    @torch.no_grad()
    def advance(self) -> Dict[Session, torch.Tensor]:
        """Every live session moves ONE forward -> `{session: latents [1, n, C, H, W]}` of the sessions whose block finished in it."""
        return self._advance(list(self.sessions))

    @torch.no_grad()
    def step(self) -> Dict[Session, torch.Tensor]:
        """`advance()` until every session live on entry has finished exactly ONE more block -> what `SessionBatch.step` returns."""
        live = list(self.sessions)
        done: Dict[Session, torch.Tensor] = {}
        todo = live
        while todo:
            done.update(self._advance(todo))
            todo = [s for s in todo if s not in done and not s.closed]
        return {s: done[s] for s in live if s in done}

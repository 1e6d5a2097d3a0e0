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

Not built (refused with the reason at construction or `open`): many-step configs, `world_size > 1`, `independent_first_frame`,
`initial_latent` / I2V, more than `max_sessions` sessions.  Out of scope: prompt changes inside a session, sessions at different
denoising steps within one forward, CausVid and MAGI, consumer threads."""
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
        self.request: Optional[KVCacheRequest] = None
        self.kv_meta: List[dict] = []
        self.cross_meta: List[dict] = []
        self.prompt_embeds: Optional[torch.Tensor] = None
        self.generator: Optional[torch.Generator] = None
        self.stream = None                  # FrameStream(num_samples=1) of a continuous=True session
        self.closed = False

    def __repr__(self):
        return f"Session({self.index}, block={self.block}{', closed' if self.closed else ''})"


class SessionBatch:
    def __init__(self, pipe, max_sessions: int = 8):
        inner = getattr(pipe, "pipeline", None)
        if getattr(pipe, "_pipeline_type", None) != "causal" or not hasattr(getattr(inner, "args", None), "denoising_step_list"):
            raise NotImplementedError("SessionBatch is built for the few-step pipeline (configs with denoising_step_list); this config "
                                      "selects the many-step CausalDiffusionInferencePipeline")
        if getattr(pipe.parallel_config, "world_size", 1) > 1:
            raise NotImplementedError(f"SessionBatch runs on one GPU: world_size {pipe.parallel_config.world_size} (ragged forwards "
                                      "are not built for sequence parallelism)")
        if getattr(inner, "independent_first_frame", False):
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

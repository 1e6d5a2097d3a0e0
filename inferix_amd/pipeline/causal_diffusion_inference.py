"""CausalDiffusionInferencePipeline — the many-step causal sampler of Self-Forcing with classifier-free guidance.

Mirror of the reference's class (inferix/pipeline/self_forcing/CausalDiffusionInferencePipeline.py:10-294), the inner pipeline that
`SelfForcingPipeline` selects for a config WITHOUT `denoising_step_list` (non-distilled, teacher-forcing and diffusion-forcing
checkpoints): per block `sampling_steps` (50) UniPC steps, each a conditional and an unconditional generator forward against two
separate KV caches (`kv_cache_manager_pos` / `kv_cache_manager_neg`), mixed with `args.guidance_scale`; then a clean-context re-run at
t = 0 on both caches.  Given frames (`initial_latent`) are prefilled into both caches at t = 0.

Here a step is ONE `generator.forward_cfg` (the two forwards as two launch chains on two streams; two `forward` calls when pairing is
off) and ONE `FlowUniPCSchedule.step_cfg` launch (ifx_cfg_unipc_step: guidance mix, x0 conversion, corrector and predictor with
host-known coefficients), with no host synchronisation inside the step loop.

Deliberate differences:
  * the reference's class never initialises `kv_cache_meta_pos` or `parallel_config` before reading them and its caller passes a
    `profile=` keyword it does not accept — as written it cannot run; the mirror initialises both and accepts the keyword;
  * the layer count and `frame_seq_length` come from the model / args, as in causal_inference.py, not from the literals 30 / 1560;
  * no per-step prints (two device reads each upstream); `kv_cache_meta` index entries are HOST tensors, as in the sibling;
  * `sample_solver = "dpm++"` and `parallel_config.world_size > 1` raise NotImplementedError (upstream hard-codes "unipc"; the
    sequence-parallel form of this sampler is not built).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Union

import torch

from ..core.types import DecodeMode
from ..kvcache_manager import KVCacheManager, KVCacheRequest
from ..schedulers import FlowUniPCSchedule
from .block_loop import BlockLoopPipeline


class CausalDiffusionInferencePipeline(BlockLoopPipeline):
    _timestep_dtype = torch.float32     # `t * torch.ones([B, F], dtype=float32)` (CausalDiffusionInferencePipeline.py:217-219)
    _timestep_cache_size = 128          # every block walks the same `sampling_steps` (50) values
    _pair_entry = "forward_cfg"         # the two forwards of a guided step, as a pair on two streams

    def __init__(self, args, device, generator=None, text_encoder=None, vae=None, parallel_config=None, profiler=None):
        super().__init__()
        if generator is None:
            from ..wan import HipWanDiffusionWrapper
            generator = HipWanDiffusionWrapper(model_path=getattr(args, "model_path", "weights/Wan2.1-T2V-1.3B"),
                                               **getattr(args, "model_kwargs", {}), is_causal=True,
                                               parallel_config=parallel_config)
        self.generator, self.text_encoder, self.vae = generator, text_encoder, vae
        self.parallel_config = parallel_config if parallel_config is not None else getattr(generator, "parallel_config", None)
        if int(getattr(self.parallel_config, "world_size", 1) or 1) > 1:
            raise NotImplementedError("CausalDiffusionInferencePipeline: parallel_config.world_size > 1 — the sequence-parallel form of "
                                      "the many-step sampler is not built")
        self._profiler = profiler
        self.device_ = torch.device(device)
        self.num_train_timesteps = getattr(args, "num_train_timestep", 1000)
        self.sampling_steps = 50
        self.sample_solver = "unipc"
        self.shift = getattr(args, "timestep_shift", 5.0)
        model = self.generator.model
        self.num_transformer_blocks = getattr(model, "num_layers", 30)
        self.frame_seq_length = getattr(args, "frame_seq_length", 1560)
        self.kv_cache_meta_pos = self.kv_cache_meta_neg = None
        self.crossattn_cache_meta_pos = self.crossattn_cache_meta_neg = None
        self._scheduler: Optional[FlowUniPCSchedule] = None
        self.args = args
        self.num_frame_per_block = getattr(args, "num_frame_per_block", 1)
        self.independent_first_frame = getattr(args, "independent_first_frame", False)
        self.local_attn_size = model.local_attn_size
        if self.num_frame_per_block > 1:
            model.num_frame_per_block = self.num_frame_per_block

    # ------------------------------------------------------------------
    def _initialize_sample_scheduler(self, noise) -> FlowUniPCSchedule:
        """A fresh solver state per block (CausalDiffusionInferencePipeline.py:364-385); the object, its coefficient table and its
        device buffers are kept from block to block."""
        if self.sample_solver == "dpm++":
            raise NotImplementedError("CausalDiffusionInferencePipeline: sample_solver 'dpm++' is not built (the reference hard-codes "
                                      "'unipc')")
        if self.sample_solver != "unipc":
            raise NotImplementedError(f"CausalDiffusionInferencePipeline: sample_solver {self.sample_solver!r}: only 'unipc' is built")
        s = self._scheduler
        if s is None or s.num_train_timesteps != self.num_train_timesteps:
            s = self._scheduler = FlowUniPCSchedule(num_train_timesteps=self.num_train_timesteps, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(self.sampling_steps, device="cpu", shift=self.shift)
        self.timesteps = s.timesteps
        return s

    def _kw(self, x, cond, timestep, start_frame, which: str, kvm, reqs) -> dict:
        return dict(noisy_image_or_video=x, conditional_dict=cond, timestep=timestep,
                    kv_cache_meta=getattr(self, "kv_cache_meta_" + which),
                    crossattn_cache_meta=getattr(self, "crossattn_cache_meta_" + which),
                    current_start=start_frame * self.frame_seq_length, kv_cache_manager=kvm, kv_cache_requests=reqs)

    def _both(self, x, cond, uncond, timestep, start_frame, kvm_pos, kvm_neg, reqs, pair: bool):
        """The conditional and the unconditional forward of the same latents: `(flow_cond, flow_uncond)`."""
        kc = self._kw(x, cond, timestep, start_frame, "pos", kvm_pos, reqs)
        ku = self._kw(x, uncond, timestep, start_frame, "neg", kvm_neg, reqs)
        if pair:
            return self.generator.forward_cfg(kc, ku)
        return self.generator(**kc)[0], self.generator(**ku)[0]

    def inference(self, noise: torch.Tensor, text_prompts: List[str], kv_cache_manager_pos: KVCacheManager,
                  kv_cache_manager_neg: KVCacheManager, kv_cache_requests: List[KVCacheRequest],
                  initial_latent: Optional[torch.Tensor] = None, return_latents: bool = False,
                  start_frame_index: Optional[int] = 0, *, profile: bool = False,
                  decode_mode: DecodeMode = DecodeMode.AFTER_ALL, block_callback: Optional[Callable] = None
                  ) -> Union[torch.Tensor, tuple]:
        B, T, Cc, Hh, Ww = noise.shape
        n_in, frames = self._block_plan(T, initial_latent)
        cond = self.text_encoder(text_prompts=text_prompts)
        uncond = self.text_encoder(text_prompts=[self.args.negative_prompt] * len(text_prompts))
        dev = noise.device
        output = torch.zeros([B, T + n_in, Cc, Hh, Ww], device=dev, dtype=noise.dtype)
        kvp, kvn, reqs = kv_cache_manager_pos, kv_cache_manager_neg, kv_cache_requests

        # ---- caches -----------------------------------------------------------------------
        if self.kv_cache_meta_pos is None:
            self._initialize_kv_cache(kvp, kvn, reqs, dtype=noise.dtype)
            self._initialize_crossattn_cache(kvp, kvn, reqs, dtype=noise.dtype)
        else:
            for metas in (self.crossattn_cache_meta_pos, self.crossattn_cache_meta_neg):
                self._reset_crossattn_meta(metas)
            for metas in (self.kv_cache_meta_pos, self.kv_cache_meta_neg):
                self._reset_kv_meta(metas)
        pair = self._pairing()

        # ---- prefill of given context frames at t = 0, into both caches ----------------------
        first = int(start_frame_index or 0)          # the window's place in a long video: offsets `current_start` only
        # `cache` counts the frames of this call: where `output`, `noise` and `initial_latent` are indexed.  One zero per frame of the
        # call where upstream hands over `[B, 1]` zeros: the same modulation for every frame, and the wrapper's x0 conversion (unused
        # here) cannot broadcast B sigmas over B * frames rows at batch > 1
        cache = self._prefill(initial_latent, output, lambda lat, done: self._both(
            lat, cond, uncond, self._timestep(0, (B, lat.shape[1]), dev, torch.int64), first + done, kvp, kvn, reqs, pair))
        cur = first + cache

        # ---- temporal (blocks) x spatial (sampling steps) loops ------------------------------
        guidance = float(self.args.guidance_scale)
        self.block_times_ms: List[float] = []
        for block_index, nf in enumerate(frames):
            if profile:
                b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b0.record()
            latents = noise[:, cache - n_in:cache + nf - n_in]
            scheduler = self._initialize_sample_scheduler(noise)
            for t in scheduler.timesteps.tolist():                   # host integers: nothing in this loop reads the device
                timestep = self._timestep(t, (B, nf), dev)
                flow_cond, flow_uncond = self._both(latents, cond, uncond, timestep, cur, kvp, kvn, reqs, pair)
                latents = scheduler.step_cfg(flow_cond, flow_uncond, guidance, t, latents, return_dict=False)[0]
            output[:, cache:cache + nf] = latents
            # clean-context re-run at t = 0 on both caches
            self._both(latents, cond, uncond, self._timestep(0, (B, nf), dev), cur, kvp, kvn, reqs, pair)
            if profile:
                b1.record()
                torch.cuda.synchronize()
                self.block_times_ms.append(b0.elapsed_time(b1))
            cur += nf
            cache += nf
            if block_callback is not None:
                block_callback(output[:, cache - nf:cache], block_index)

        self._finish(output, "CausalDiffusionInferencePipeline.inference")
        if decode_mode == DecodeMode.NO_DECODE:
            return (output, output) if return_latents else output
        if self.vae is None or not hasattr(self.vae, "decode_to_pixel"):
            raise RuntimeError("decode requested but no VAE with decode_to_pixel() was injected")
        return self._to_video(output, return_latents)

    # ------------------------------------------------------------------
    @property
    def _cache_blocks(self):
        blocks = self.generator.model.blocks
        return [blocks[l] for l in range(self.num_transformer_blocks)]

    def _initialize_kv_cache(self, kv_cache_manager_pos, kv_cache_manager_neg, kv_cache_requests, dtype):
        size = self.local_attn_size * self.frame_seq_length if self.local_attn_size != -1 \
            else getattr(self.args, "kv_cache_tokens", 32760)
        self._walk_caches("allocate_kv_cache", (kv_cache_manager_pos, kv_cache_manager_neg), kv_cache_requests, sequence_length=size,
                          dtype=dtype, ulysses_size=1, ring_size=1)
        self.kv_cache_meta_pos = self._fresh_kv_meta(self.num_transformer_blocks)
        self.kv_cache_meta_neg = self._fresh_kv_meta(self.num_transformer_blocks)

    def _initialize_crossattn_cache(self, kv_cache_manager_pos, kv_cache_manager_neg, kv_cache_requests, dtype):
        self._walk_caches("allocate_crossattn_cache", (kv_cache_manager_pos, kv_cache_manager_neg), kv_cache_requests,
                          crossattn_length=getattr(self.generator.model, "text_len", 512), dtype=dtype)
        self.crossattn_cache_meta_pos = self._fresh_crossattn_meta(self.num_transformer_blocks)
        self.crossattn_cache_meta_neg = self._fresh_crossattn_meta(self.num_transformer_blocks)

    def clear_cache(self, kv_cache_manager_pos, kv_cache_manager_neg, kv_cache_requests):
        self._walk_caches("clear_cache", (kv_cache_manager_pos, kv_cache_manager_neg), kv_cache_requests)
        self.kv_cache_meta_pos = self.kv_cache_meta_neg = None
        self.crossattn_cache_meta_pos = self.crossattn_cache_meta_neg = None

"""BlockLoopPipeline — what the three Wan inner pipelines (causal_inference.py, causvid_inference.py, causal_diffusion_inference.py)
share around their step loops: the denoising-step tensor, the constant-timestep cache, the pairing switch, the per-layer cache walks,
the cache meta lists, the block plan, the prefill of given frames, the end-of-clip checks and the decode.  Each piece exists once,
here; the step loops themselves (few-step with re-noising, CausVid's, the guided UniPC one) stay in their classes."""
from __future__ import annotations

import contextlib
import os
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from ..schedulers import const_timestep


class BlockLoopPipeline(torch.nn.Module):
    _timestep_dtype = torch.int64       # default dtype of `_timestep`
    _timestep_cache_size = 32           # distinct (value, shape, device, dtype) a clip walks, with room
    _pair_entry = "forward_pair"        # the generator method `_pairing` needs

    def __init__(self):
        super().__init__()
        self._ts_cache: dict = {}

    # ---- constants of a clip ----------------------------------------------------------------------
    @staticmethod
    def _denoising_steps(args, scheduler, drop_last: bool = False) -> torch.Tensor:
        """`args.denoising_step_list` as a long tensor (CausVid drops the last entry), mapped through the scheduler's timestep table
        when `args.warp_denoising_step` is set."""
        steps = torch.tensor(list(args.denoising_step_list), dtype=torch.long)
        if drop_last:
            steps = steps[:-1]
        if getattr(args, "warp_denoising_step", False):
            ts = torch.cat((scheduler.timesteps.cpu(), torch.tensor([0], dtype=torch.float32)))
            steps = ts[1000 - steps]
        return steps

    def _timestep(self, value, shape, device, dtype=None) -> torch.Tensor:
        """`torch.ones(shape) * value` (CausalInferencePipeline.py:330,371; CausalDiffusionInferencePipeline.py:217-219), ONE tensor per
        (value, shape) reused across blocks: the model and the x0 / add_noise conversions memoise what they derive from a timestep
        tensor (the modulation tables, the sigma lookups) on the scalar it holds — `schedulers.const_timestep` tags the tensor with it —
        ~25 glue launches per forward less.  A tagged tensor is a constant: never written, in place or through a raw pointer."""
        dtype = self._timestep_dtype if dtype is None else dtype
        key = (float(value), tuple(shape), str(device), dtype)
        t = self._ts_cache.get(key)
        if t is None:
            if len(self._ts_cache) >= self._timestep_cache_size:
                self._ts_cache.clear()
            t = self._ts_cache[key] = const_timestep(value, shape, device, dtype)
        return t

    def _pairing(self) -> bool:
        """Whether two generator forwards are enqueued TOGETHER on two streams through the generator's `_pair_entry`.  `forward_pair`:
        the clean-context re-run of block b with the first denoising step of block b + 1, layer by layer — the two calls depend on
        each other only through layer l's cache rows, so the second chain's launches fill the tails and the dependent-launch gaps of the
        first (- 2 .. 3 % of a clip on one GPU, - 4 .. 5 % on an emulated sequence-parallel rank).  `forward_cfg`: the
        conditional and the unconditional forward of a guided step.  Either way the results are bit-identical to the sequential calls
        (tests/test_hip_model.py, tests/test_hip_causal_diffusion.py).  `args.pair_forwards` / env IFX_PAIR_FORWARDS: 1 on, 0 off;
        unset = on.  Read at call time: the benchmark flips `args.pair_forwards` on a live pipeline."""
        if not hasattr(self.generator, self._pair_entry):
            return False
        want = getattr(self.args, "pair_forwards", None)
        if want is None and os.environ.get("IFX_PAIR_FORWARDS", "") != "":
            want = os.environ["IFX_PAIR_FORWARDS"] not in ("0", "false", "off")
        return True if want is None else bool(want)

    # ---- caches --------------------------------------------------------------------------------------
    def _walk_caches(self, method: str, managers: Sequence, requests: Sequence, **kw) -> None:
        """`blk.kv_cache_manager.<method>(...)` for every (block of `_cache_blocks`, request, manager), in that nesting."""
        for blk in self._cache_blocks:
            for req in requests:
                for kvm in managers:
                    getattr(blk.kv_cache_manager, method)(kv_cache_manager=kvm, kv_cache_request=req, **kw)

    @staticmethod
    def _fresh_kv_meta(n: int) -> List[dict]:
        """The index entries are HOST tensors: the slot arithmetic runs on the host."""
        return [{"global_end_index": torch.tensor([0], dtype=torch.long), "local_end_index": torch.tensor([0], dtype=torch.long)}
                for _ in range(n)]

    @staticmethod
    def _fresh_crossattn_meta(n: int) -> List[dict]:
        return [{"is_init": False} for _ in range(n)]

    @staticmethod
    def _reset_kv_meta(metas: List[dict]) -> None:
        for m in metas:
            m["global_end_index"] = torch.tensor([0], dtype=torch.long)
            m["local_end_index"] = torch.tensor([0], dtype=torch.long)

    @staticmethod
    def _reset_crossattn_meta(metas: List[dict]) -> None:
        for m in metas:
            m["is_init"] = False

    # ---- the clip ------------------------------------------------------------------------------------
    def _block_plan(self, T: int, initial_latent: Optional[torch.Tensor]) -> Tuple[int, List[int]]:
        """`(n_in, frames)`: the given frames in front of the clip, and the frame count of every block to generate."""
        nfb = self.num_frame_per_block
        if not self.independent_first_frame or initial_latent is not None:
            assert T % nfb == 0
            frames = [nfb] * (T // nfb)
        else:
            assert (T - 1) % nfb == 0
            frames = [1] + [nfb] * ((T - 1) // nfb)
        return (initial_latent.shape[1] if initial_latent is not None else 0), frames

    def _prefill(self, initial_latent: Optional[torch.Tensor], output: torch.Tensor, call: Callable) -> int:
        """The given context frames copied into `output` and run through `call(latents, frames_done)` (each class's own forward at
        t = 0): the independent first frame alone, then block by block.  Returns the number of frames done."""
        if initial_latent is None:
            return 0
        nfb, n_in, done = self.num_frame_per_block, initial_latent.shape[1], 0
        if self.independent_first_frame:
            assert (n_in - 1) % nfb == 0
            n_pref = (n_in - 1) // nfb
            output[:, :1] = initial_latent[:, :1]
            call(initial_latent[:, :1], 0)
            done = 1
        else:
            assert n_in % nfb == 0
            n_pref = n_in // nfb
        for _ in range(n_pref):
            ref = initial_latent[:, done:done + nfb]
            output[:, done:done + nfb] = ref
            call(ref, done)
            done += nfb
        return done

    def _finish(self, output: torch.Tensor, what: str) -> None:
        """The end of a clip, before it is handed out."""
        cp = getattr(getattr(self.generator, "model", None), "cp", None)
        if cp is not None and hasattr(cp, "check_now"):
            cp.check_now()             # a sequence-parallel rank: a peer-store wait that gave up is reported before the clip is handed out
        if output.is_cuda:
            from .. import hip_ops
            hip_ops.check_device(what, sync=True)    # a split-K wait that gave up: the clip is garbage — raise, do not ship it

    def _to_video(self, output: torch.Tensor, return_latents: bool, context=None, **decode_kw):
        """Latents to pixels in [0, 1] (the decode inside `context`, when one is given): `video`, or `(video, latents)`."""
        with context if context is not None else contextlib.nullcontext():
            video = self.vae.decode_to_pixel(output, **decode_kw)
        video = (video * 0.5 + 0.5).clamp(0, 1)
        return (video, output) if return_latents else video

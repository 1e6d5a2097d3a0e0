"""MAGI's chunk schedule: which chunks a denoise forward carries, at which timesteps, over which key ranges.

Host mirror of the planning half of `SampleTransport` (inferix/pipeline/magi/video_generate.py):
  generate_sequences                         :166-182   per-stage chunk window and timestep window
  init_t / init_intervel                     :185-236   the time grid (sd3 / square / piecewise / identity) and distill intervals
  get_timestep / get_denoise_step_of_each_chunk :324-359
  generate_denoise_status_and_sequences      :554-572
  total_forward_step                         :574-585
  forward_velocity (steps 3-7)               :587-668   slice_point / range_num / denoising_range_num, the extra clean chunk, kv ranges
  integrate                                  :531-552   x += v * (t[i + 1] - t[i]) per chunk

Pure integer / small-tensor work on the host: `ChunkSchedule.plan(step)` is everything `forward_velocity` computes before it calls the
model, `ChunkSchedule.run(model, ...)` is the reference's forward_velocity + integrate_velocity loop for one clip, with or without a
prefix video (`extract_prefix_video_feature` / `try_pad_prefix_video`, :391-454).  tests/test_magi_schedule.py checks plans, timesteps and key ranges against a golden the reference's
own methods produced for every step of the 4.5B distill configuration.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .kv_ranges import chunk_token_nums, generate_kvrange_for_denoising_video
from .types import RangePlan


def generate_sequences(chunk_num: int, window_size: int, chunk_offset: int) -> Tuple[List[int], List[int], List[int], List[int]]:
    """Stage i (one per chunk entering or leaving the window) denoises chunks [clip_start[i], clip_end[i]) whose positions inside the
    window are [t_start[i], t_end[i])."""
    stages = range(chunk_offset, chunk_num + window_size - 1)
    clip_start = [max(chunk_offset, i - window_size + 1) for i in stages]
    clip_end = [min(chunk_num, i + 1) for i in stages]
    t_start = [max(0, i - chunk_num + 1) for i in stages]
    t_end = [min(window_size, i - chunk_offset + 1) for i in stages]
    return clip_start, clip_end, t_start, t_end


def init_t(t_schedule_config: Optional[Dict], num_steps: int, device="cpu", shortcut_mode: str = "") -> torch.Tensor:
    """The time grid t[0 .. num_steps] (0: noise, 1: clean)."""
    cfg = t_schedule_config or {}
    if num_steps == 12:
        base = torch.linspace(0, 1, 5, device=device) / 4
        accu = torch.linspace(0, 1, 5, device=device)
        base = base[:3] if shortcut_mode == "16,16,8" else torch.cat([base[:1], base[2:4]], dim=0)
        t = torch.cat([base + a for a in accu], dim=0)[: num_steps + 1]
    else:
        t = torch.linspace(0, 1, num_steps + 1, device=device)
    func = cfg.get("tSchedulerFunc", "sd3")
    if func == "sd3":
        shift = cfg.get("shift", 3.0)
        assert shift >= 1.0, "shift should >=1"
        inv = 1.0 / shift
        t = t ** 2
        t = inv * t / (1 + (inv - 1) * t)
    elif func == "square":
        t = t ** 2
    elif func == "piecewise":
        low = t < 0.875
        t = torch.where(low, t * (0.5 / 0.875), 0.5 + (t - 0.875) * (0.5 / (1 - 0.875)))
    return t


def init_interval(num_steps: int, device="cpu", shortcut_mode: str = "") -> torch.Tensor:
    if num_steps % 3 == 0:
        pat = [1, 1, 2] if shortcut_mode == "16,16,8" else [2, 1, 1]
        return torch.tensor(pat * (num_steps // 3), device=device)
    return torch.ones(num_steps, device=device)


# ---- what a step needs on the host: pure functions of one host copy of the time grid ---------------------------------------------------
# `ChunkSchedule.walk` reads `init_t`'s grid off the device once per clip (`host_grid`); timesteps, dt, the nearly-clean decision, the
# guidance bins and weights of every step then come from these, in the same fp32 arithmetic the device-side formulas of `run` and
# `_dispatch_3cfg` use, so no step waits for the device.
def host_grid(t_total: torch.Tensor, interval: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    """The clip's ONE device read: `(t_total, interval)` as fp32 host arrays (one copy for both)."""
    both = torch.cat([t_total.to(torch.float32), interval.to(torch.float32)]).cpu().numpy()
    return both[:t_total.numel()].copy(), both[t_total.numel():].copy()


def prefix_clean_chunks(prefix_frames: int, slice_point: int, chunk_width: int) -> int:
    """try_pad_prefix_video (:437-454): how many leading ranges of a forward are whole prefix chunks (their timestep becomes 1)."""
    start = slice_point * chunk_width
    return (prefix_frames - start) // chunk_width if prefix_frames > start else 0


def step_timesteps(t_host: np.ndarray, plan: "ForwardPlan", clean_t: float, clean_chunks: int = 0) -> np.ndarray:
    """`ChunkSchedule.timestep` + the `t[:, :clean] = 1.0` rule: one fp32 time per range of the forward, the clean chunk's in front."""
    t = t_host[list(plan.t_index)].astype(np.float32)
    if plan.fwd_extra_1st_chunk:
        t = np.concatenate([np.asarray([clean_t], np.float32), t])
    if clean_chunks > 0:
        t[:clean_chunks] = 1.0
    return t


def step_dt(t_host: np.ndarray, plan: "ForwardPlan") -> np.ndarray:
    """integrate (:542-544): t[i + 1] - t[i] per denoising chunk, an fp32 subtraction."""
    idx = np.asarray(plan.t_index, np.int64)
    return (t_host[idx + 1] - t_host[idx]).astype(np.float32)


def nearly_clean(t_row: np.ndarray, plan: "ForwardPlan", threshold: float) -> bool:
    """forward_velocity (:640-644): the first denoising chunk's time against `distill_nearly_clean_chunk_threshold`."""
    return float(t_row[int(plan.fwd_extra_1st_chunk)]) > threshold


def nearly_clean_weights(scale: float) -> Tuple[float, float]:
    """The blend of the nearly-clean re-forward (dit_model.py:563-566): `scale`, and `1 - scale` formed in double as Python forms it,
    each rounded to fp32 where the tensor operator takes it."""
    return float(np.float32(scale)), float(np.float32(1 - scale))


def cfg_bins(t_chunks: np.ndarray, cfg_t_range: Sequence[float]) -> List[int]:
    """get_cfg_scale (dit_model.py:494-497): `searchsorted(cfg_t_range - 1e-7, t) - 1` per denoising chunk, the edges shifted in fp32."""
    edges = np.asarray(cfg_t_range, np.float32) - np.float32(1e-7)
    bins = (np.searchsorted(edges, np.asarray(t_chunks, np.float32), side="left") - 1).tolist()
    assert all(0 <= b < len(cfg_t_range) for b in bins), f"a timestep of {list(t_chunks)} lies outside cfg_t_range {list(cfg_t_range)}"
    return bins


def cfg_weights(bins: Sequence[int], prev_chunk_scales: Sequence[float], text_scales: Sequence[float]
                ) -> Tuple[List[float], List[float], List[float]]:
    """The three guidance weights per chunk (dit_model.py:517-527), `(1 - s_prev, s_prev - s_text, s_text)` on
    `(uncond, cond_pre, cond_pre_and_text)`, each an fp32 operation on the fp32 scales."""
    sp = np.asarray(prev_chunk_scales, np.float32)[list(bins)]
    st = np.asarray(text_scales, np.float32)[list(bins)]
    return (np.float32(1) - sp).tolist(), (sp - st).tolist(), st.tolist()


def hand_out(chunk_start: int, denoise_count: int, num_steps: int, chunk_width: int, chunk_offset: int, prefix_frames: int
             ) -> Optional[Tuple[int, int, int]]:
    """integrate_velocity's hand-out rule (:695-721): after a step that brought chunk `chunk_start` to `denoise_count` integrations,
    `(chunk index behind the prefix, first frame, end frame)` of what is handed out, or None.  A chunk wholly inside the prefix is not
    handed out; one the prefix reaches into starts at the prefix's end — except the image case (a 1-frame prefix), which keeps frame 0."""
    if denoise_count != num_steps:
        return None
    end = (chunk_start + 1) * chunk_width
    start = chunk_start * chunk_width
    if prefix_frames > 0:
        if end <= prefix_frames:
            return None
        start = max(start, prefix_frames)
        if chunk_start == 0 and prefix_frames == 1:
            start = 0
    return chunk_start - chunk_offset, start, end


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    """Host tensor -> device through pinned memory, without waiting for the device."""
    return t.pin_memory().to(device, non_blocking=True)


@dataclass
class ForwardPlan:
    """What one `forward_velocity` call hands to the model."""
    step: int
    denoise_step_per_stage: int
    denoise_stage: int
    denoise_idx: int
    chunk_start: int
    chunk_end: int
    t_start: int
    t_end: int
    fwd_extra_1st_chunk: bool
    slice_point: int
    range_num: int
    denoising_range_num: int
    t_index: List[int]                       # rows of the time grid, one per denoising chunk (without the clean chunk's entry)
    denoise_step_of_each_chunk: List[int]    # with num_steps in front for the clean chunk


class ChunkSchedule:
    """The schedule of one clip: `chunk_num` chunks of `chunk_width` latent frames, `window_size` of them in flight."""

    def __init__(self, num_steps: int, window_size: int, chunk_num: int, chunk_width: int, chunk_offset: int = 0):
        assert num_steps % window_size == 0
        self.num_steps, self.window_size, self.chunk_num, self.chunk_width = num_steps, window_size, chunk_num, chunk_width
        self.chunk_offset = chunk_offset
        self.seq = generate_sequences(chunk_num, window_size, chunk_offset)

    def total_forward_step(self) -> int:
        return (self.num_steps // self.window_size) * (self.chunk_num + self.window_size - 1 - self.chunk_offset)

    def plan(self, step: int) -> ForwardPlan:
        per = self.num_steps // self.window_size
        stage, idx = step // per, step % per
        cs, ce, ts, te = (s[stage] for s in self.seq)
        extra = cs > self.chunk_offset and idx == 0
        t_index = [i * per + idx for i in range(ts, te)][::-1]
        steps = ([self.num_steps] if extra else []) + t_index
        return ForwardPlan(step=step, denoise_step_per_stage=per, denoise_stage=stage, denoise_idx=idx, chunk_start=cs, chunk_end=ce,
                           t_start=ts, t_end=te, fwd_extra_1st_chunk=extra, slice_point=cs - 1 if extra else cs, range_num=ce,
                           denoising_range_num=ce - cs + (1 if extra else 0), t_index=t_index, denoise_step_of_each_chunk=steps)

    def timestep(self, t_total: torch.Tensor, plan: ForwardPlan, clean_t: float, advance: int = 0) -> torch.Tensor:
        """get_timestep: the chunks' times, newest chunk last; the clean chunk (if any) in front at `clean_t`."""
        t = t_total[[i + advance for i in plan.t_index]]
        if plan.fwd_extra_1st_chunk and advance == 0:
            t = torch.cat([torch.ones(1, device=t.device) * clean_t, t], 0)
        return t

    def kv_range(self, plan: ForwardPlan, tokens: int, noise2clean_kvrange: Sequence[int], clean_chunk_kvrange: int,
                 device="cpu") -> torch.Tensor:
        return generate_kvrange_for_denoising_video(tokens, plan.slice_point, plan.denoising_range_num, plan.denoise_step_of_each_chunk,
                                                    self.num_steps, noise2clean_kvrange, clean_chunk_kvrange, 1, device)

    def extract_prefix_video_feature(self, model, prefix_video, y, emb_masks, inference_params, tokens: int, distill_interval,
                                     caption_lens: Optional[np.ndarray] = None) -> None:
        """One forward over the prefix video's whole chunks for the sake of its KV-cache writes (:391-435).  `caption_lens` (`walk`): the
        host copy `[2, chunk_num]` of the caption lengths — the key ranges then go up through pinned memory and the forward takes a
        `RangePlan`, so the pass does not wait for the device."""
        from .kv_ranges import generate_kvrange_for_prefix_video
        rc, off, cw = model.runtime_config, self.chunk_offset, self.chunk_width
        xc = prefix_video[:, :, :off * cw]
        if xc.shape[0] == 1:
            xc = torch.cat([xc, xc], 0)
        null_y = torch.cat([y[1:2, :off], y[1:2, :off]], 0)                   # clean feature without y embedding
        null_m = torch.cat([emb_masks[1:2, :off], emb_masks[1:2, :off]], 0)
        t = (torch.ones(off, device=xc.device) * rc.clean_t).unsqueeze(0).repeat(xc.size(0), 1)
        extra = {}
        if caption_lens is None:
            kv = generate_kvrange_for_prefix_video(tokens, off, rc.noise2clean_kvrange, rc.clean_chunk_kvrange, 1, xc.device)
        else:
            kv_host = generate_kvrange_for_prefix_video(tokens, off, rc.noise2clean_kvrange, rc.clean_chunk_kvrange, 1, "cpu")
            kv = _upload(kv_host, xc.device)
            extra["range_plan"] = RangePlan.make(kv_host.numpy(), list(caption_lens[1, :off]) * 2)
            if getattr(rc, "cfg_number", None) == 3:      # the dispatcher's own check of the guidance bins reads the device: made here, on the host
                cfg_bins(np.full(off, rc.clean_t, np.float32), rc.cfg_t_range)
        model.forward_dispatcher(x=xc, timestep=t, y=null_y.flatten(0, 1).unsqueeze(1), mask=null_m.flatten(0, 1).unsqueeze(1), kv_range=kv,
                                 inference_params=inference_params, chunk_width=cw, num_steps=self.num_steps, slice_point=0, range_num=off,
                                 denoising_range_num=off, fwd_extra_1st_chunk=False, extract_prefix_video_feature=True,
                                 distill_interval=distill_interval, **extra)

    # ---- the loop -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def run(self, model, x: torch.Tensor, y: torch.Tensor, emb_masks: torch.Tensor, inference_params, t_schedule_config=None,
            steps: Optional[Sequence[int]] = None, on_forward=None, prefix_video: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward_velocity + integrate_velocity for every step (or the listed `steps`) of one clip.
        x `[2 N, C, T, H, W]` noise (both halves equal, as upstream's `torch.cat([x, x])`), y `[2, chunk_num, L, C]` caption
        embeddings (row 1: the null caption), emb_masks `[2, chunk_num, L]`.  `prefix_video` `[2 N, C, Tp, H, W]` clean latents in front
        (image / video continuation; the schedule must have been built with `chunk_offset = Tp // chunk_width`): its whole chunks go
        through the model once, at clean_t with the null caption, to fill the KV cache (`extract_prefix_video_feature`, :391-435), and
        every forward has the prefix frames it overlaps pasted over its noise at t = 1 (`try_pad_prefix_video`, :437-454).
        Returns x denoised in place."""
        rc, ec, mc = model.runtime_config, model.engine_config, model.model_config
        dev = x.device
        if (prefix_video.size(2) // self.chunk_width if prefix_video is not None else 0) != self.chunk_offset:
            raise ValueError(f"the schedule was built for chunk_offset {self.chunk_offset}, the prefix video holds "
                             f"{0 if prefix_video is None else prefix_video.size(2) // self.chunk_width} whole chunks")
        shortcut = getattr(ec, "shortcut_mode", "")
        t_total = init_t(t_schedule_config or {}, self.num_steps, dev, shortcut)
        interval = init_interval(self.num_steps, dev, shortcut)
        tokens = chunk_token_nums(self.chunk_width, x.shape[3], x.shape[4], getattr(mc, "patch_size", 2))
        cw = self.chunk_width
        for step in (range(self.total_forward_step()) if steps is None else steps):
            p = self.plan(step)
            xc = x[:, :, p.chunk_start * cw: p.chunk_end * cw].clone()
            yc, mk = y[:, p.chunk_start:p.chunk_end], emb_masks[:, p.chunk_start:p.chunk_end]
            if p.fwd_extra_1st_chunk:
                xc = torch.cat([x[:, :, (p.chunk_start - 1) * cw: p.chunk_start * cw].clone(), xc], dim=2)
                yc = torch.cat([y[1:2, 0:1].expand(yc.size(0), -1, -1, -1), yc], dim=1)          # clean feature without y embedding
                mk = torch.cat([emb_masks[1:2, 1:2].expand(mk.size(0), -1, -1), mk], dim=1)
            if self.chunk_offset > 0 and step == 0:
                self.extract_prefix_video_feature(model, prefix_video, y, emb_masks, inference_params, tokens, interval[0])
            t = self.timestep(t_total, p, rc.clean_t).unsqueeze(0).repeat(xc.size(0), 1)
            kv = self.kv_range(p, tokens, rc.noise2clean_kvrange, rc.clean_chunk_kvrange, dev)
            if prefix_video is not None:                                      # try_pad_prefix_video
                start = p.slice_point * cw
                if prefix_video.size(2) > start:
                    n = min(prefix_video.size(2) - start, xc.size(2))
                    xc[:, :, :n] = prefix_video[:, :, start:start + n]
                    clean = (prefix_video.size(2) - start) // cw
                    if clean > 0:
                        t[:, :clean] = 1.0
            nearly_clean_t = t[0, int(p.fwd_extra_1st_chunk)].item()
            kwargs = dict(chunk_width=cw, fwd_extra_1st_chunk=p.fwd_extra_1st_chunk, num_steps=self.num_steps, slice_point=p.slice_point,
                          range_num=p.range_num, denoising_range_num=p.denoising_range_num,
                          distill_nearly_clean_chunk=nearly_clean_t > getattr(ec, "distill_nearly_clean_chunk_threshold", 0.3),
                          distill_interval=interval[p.denoise_idx])
            v = model.forward_dispatcher(x=xc, timestep=t, y=yc.flatten(0, 1).unsqueeze(1), mask=mk.flatten(0, 1).unsqueeze(1),
                                         kv_range=kv, inference_params=inference_params, **kwargs)
            if on_forward is not None:
                on_forward(p)
            if p.fwd_extra_1st_chunk:
                xc, v = xc[:, :, cw:], v[:, :, cw:]
            dt = self.timestep(t_total, p, rc.clean_t, advance=1) - t_total[p.t_index]
            N, C, T, H, W = xc.shape
            xc = (xc.reshape(N, C, -1, cw, H, W) + v.reshape(N, C, -1, cw, H, W) * dt.reshape(1, 1, -1, 1, 1, 1)).reshape(N, C, T, H, W)
            x[:, :, p.chunk_start * cw: p.chunk_end * cw] = xc
        return x

    def hand_outs(self, prefix_frames: int = 0) -> List[Optional[Tuple[int, int, int]]]:
        """`hand_out` for every forward step of the clip, in order: what `walk` yields behind each step (None: nothing)."""
        counts = [0] * self.chunk_num
        out = []
        for step in range(self.total_forward_step()):
            p = self.plan(step)
            for c in range(p.chunk_start, p.chunk_end):
                counts[c] += 1
            out.append(hand_out(p.chunk_start, counts[p.chunk_start], self.num_steps, self.chunk_width, self.chunk_offset, prefix_frames))
        return out

    @torch.no_grad()
    def walk(self, model, x: torch.Tensor, y: torch.Tensor, emb_masks: torch.Tensor, inference_params, t_schedule_config=None,
             prefix_video: Optional[torch.Tensor] = None, host_plans: bool = True):
        """`SampleTransport.walk` (:723-756) for one clip: the steps of `run`, in the same order and with the same model inputs, as a
        generator that hands out every chunk the moment its last step is integrated — `(chunk index behind the prefix, view
        x[0:1, :, first:end])`, enqueued on the current stream; later steps never write those frames.  Arguments as `run`; x fp32 on
        the GPU, denoised in place, both rows kept equal (the rows of x and of `prefix_video` are equal on entry, as upstream's
        `torch.cat([x, x])`: the step reads row 0 and stores both).

        Per step: `model.forward_velocities` (the forwards of `forward_dispatcher` without its mixing) and ONE `ifx_magi_integrate`
        launch (guidance mix + Euler step).  The time grid is read off the device once, before the first forward (`host_grid`); every
        scalar a step needs is derived from that copy on the host, and the tensors it builds there reach the device through pinned
        memory: between the first forward and the last, nothing here waits for the device.

        Nor does the model: the caption lengths ride in the same one read as the time grid, and every forward is handed a `RangePlan`
        (its key ranges and caption lengths as the host knows them), on which `HipVideoDiTModel` builds its packed ranges without
        reading them back.  `host_plans=False` withholds the plans: the model then recovers the ranges from the device tensors at the
        head of every forward, the same results with one wait per forward.  Captions whose valid tokens are not their first ones
        (a mask with holes) get no plan either."""
        from .. import hip_ops as ops
        rc, ec, mc = model.runtime_config, model.engine_config, model.model_config
        dev, cw = x.device, self.chunk_width
        prefix_frames = prefix_video.size(2) if prefix_video is not None else 0
        if prefix_frames // cw != self.chunk_offset:
            raise ValueError(f"the schedule was built for chunk_offset {self.chunk_offset}, the prefix video holds "
                             f"{prefix_frames // cw} whole chunks")
        shortcut = getattr(ec, "shortcut_mode", "")
        t_total = init_t(t_schedule_config or {}, self.num_steps, dev, shortcut)
        interval = init_interval(self.num_steps, dev, shortcut)
        # the clip's one read: the time grid, and behind it the caption lengths [2, chunk_num] and whether any mask has a hole
        valid = emb_masks != 0
        holes = (valid[..., 1:] & ~valid[..., :-1]).any().reshape(1)
        t_host, tail = host_grid(t_total, torch.cat([interval.to(torch.float32), valid.sum(-1).flatten().to(torch.float32),
                                                     holes.to(torch.float32)]))
        lens = None
        if host_plans and tail[-1] == 0:
            lens = tail[interval.numel():-1].astype(np.int64).reshape(emb_masks.shape[0], emb_masks.shape[1])
        tokens = chunk_token_nums(cw, x.shape[3], x.shape[4], getattr(mc, "patch_size", 2))
        threshold = getattr(ec, "distill_nearly_clean_chunk_threshold", 0.3)
        three = getattr(rc, "cfg_number", None) == 3
        plans = [self.plan(step) for step in range(self.total_forward_step())]
        rows = [step_timesteps(t_host, p, rc.clean_t, prefix_clean_chunks(prefix_frames, p.slice_point, cw)) for p in plans]
        table = np.zeros((max(len(plans), 1), self.window_size + 1), np.float32)
        for i, r in enumerate(rows):
            table[i, :len(r)] = r
        t_table = _upload(torch.from_numpy(table), dev)                      # every step's timestep row, one upload per clip
        outs = self.hand_outs(prefix_frames)
        for step, p in enumerate(plans):
            xc = x[:, :, p.chunk_start * cw: p.chunk_end * cw].clone()
            yc, mk = y[:, p.chunk_start:p.chunk_end], emb_masks[:, p.chunk_start:p.chunk_end]
            if p.fwd_extra_1st_chunk:
                xc = torch.cat([x[:, :, (p.chunk_start - 1) * cw: p.chunk_start * cw].clone(), xc], dim=2)
                yc = torch.cat([y[1:2, 0:1].expand(yc.size(0), -1, -1, -1), yc], dim=1)          # clean feature without y embedding
                mk = torch.cat([emb_masks[1:2, 1:2].expand(mk.size(0), -1, -1), mk], dim=1)
            if self.chunk_offset > 0 and step == 0:
                self.extract_prefix_video_feature(model, prefix_video, y, emb_masks, inference_params, tokens, interval[0], caption_lens=lens)
            row = rows[step]
            t = t_table[step, :len(row)].unsqueeze(0).repeat(xc.size(0), 1)
            kv_host = self.kv_range(p, tokens, rc.noise2clean_kvrange, rc.clean_chunk_kvrange, "cpu")
            kv = _upload(kv_host, dev)
            plan = {}
            if lens is not None:                                              # the rows of `mk`, flattened: both caption rows of every range
                ml = lens[:, p.chunk_start:p.chunk_end]
                if p.fwd_extra_1st_chunk:
                    ml = np.concatenate([np.full((ml.shape[0], 1), lens[1, 1]), ml], axis=1)
                plan["range_plan"] = RangePlan.make(kv_host.numpy(), ml.reshape(-1))
            start = p.slice_point * cw
            if prefix_frames > start:                                         # try_pad_prefix_video
                n = min(prefix_frames - start, xc.size(2))
                xc[:, :, :n] = prefix_video[:, :, start:start + n]
                a = p.chunk_start * cw                                        # the step integrates the clip in place: the frames of the
                if start + n > a:                                             # window (not the clean chunk in front) take the paste too
                    x[:, :, a:start + n] = prefix_video[:, :, a:start + n]
            n_dn = p.chunk_end - p.chunk_start
            kwargs = dict(chunk_width=cw, fwd_extra_1st_chunk=p.fwd_extra_1st_chunk, num_steps=self.num_steps, slice_point=p.slice_point,
                          range_num=p.range_num, denoising_range_num=p.denoising_range_num, distill_interval=interval[p.denoise_idx])
            sources = model.forward_velocities(x=xc, timestep=t, y=yc.flatten(0, 1).unsqueeze(1), mask=mk.flatten(0, 1).unsqueeze(1),
                                               kv_range=kv, inference_params=inference_params,
                                               nearly_clean=nearly_clean(row, p, threshold),
                                               cfg_bins=cfg_bins(row[-n_dn:], rc.cfg_t_range) if three else None, **kwargs, **plan)
            ops.magi_integrate(x, p.chunk_start, cw, step_dt(t_host, p).tolist(), sources)
            out = outs[step]
            if out is not None:
                yield out[0], x[0:1, :, out[1]:out[2]]


def generate_per_chunk(model, prefix_video: Optional[torch.Tensor], caption_embs: torch.Tensor, emb_masks: torch.Tensor, *,
                       noise: Optional[torch.Tensor] = None):
    """`generate_per_chunk` (:759-769): `extract_feature_for_inference` -> noise `torch.randn(*latent_size)` duplicated to two rows ->
    `InferenceParams(1, T H/p W/p)` -> the schedule of `runtime_config` (`num_steps`, `window_size`, `chunk_width`; `chunk_offset` from
    the prefix) -> the chunk tensors of `ChunkSchedule.walk`, each `[1, C, frames, H, W]`, then `dist.barrier()` when a process group
    exists.  `noise` `[1, C, T, H, W]` replaces the random draw (tests).  Pipeline parallelism is not built (`engine_config.pp_size`
    > 1 is refused).  Upstream's `gc.collect()` / `torch.cuda.empty_cache()` behind the loop is allocator hygiene for small cards and
    is not mirrored: it would hand 288 GB of cached blocks back only to ask for them again at the next request."""
    import torch.distributed as dist
    from .prompt import extract_feature_for_inference
    from .types import InferenceParams
    rc, ec, mc = model.runtime_config, model.engine_config, model.model_config
    if getattr(ec, "pp_size", 1) > 1:
        raise NotImplementedError("generate_per_chunk: pipeline parallelism (engine_config.pp_size > 1) is not built")
    dev = torch.device(model.device)
    if prefix_video is not None:
        prefix_video = prefix_video.to(dev)
    inp = extract_feature_for_inference(model, prefix_video, caption_embs, emb_masks)
    if noise is None:
        noise = torch.randn(*inp.latent_size, device=dev)
    elif tuple(noise.shape) != tuple(inp.latent_size):
        raise ValueError(f"noise has shape {tuple(noise.shape)}, the request's latent size is {tuple(inp.latent_size)}")
    noise = noise.to(dev, torch.float32)
    x = torch.cat([noise, noise], 0)
    _, _, T, H, W = inp.latent_size
    patch = getattr(mc, "patch_size", 2)
    params = InferenceParams(1, T * (H // patch) * (W // patch), device=dev)
    prefix = None
    if prefix_video is not None:
        prefix = torch.cat([prefix_video, prefix_video], 0) if prefix_video.size(0) == 1 else prefix_video
    sch = ChunkSchedule(inp.num_steps, rc.window_size, inp.chunk_num, rc.chunk_width,
                        chunk_offset=(prefix.size(2) // rc.chunk_width) if prefix is not None else 0)
    for _, chunk in sch.walk(model, x, inp.y.to(dev), inp.emb_masks.to(dev), params, inp.t_schedule_config, prefix_video=prefix):
        yield chunk
    if dist.is_available() and dist.is_initialized():
        dist.barrier()

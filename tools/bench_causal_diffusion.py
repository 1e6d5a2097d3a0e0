#!/usr/bin/env python3
"""What the many-step guided causal sampler (`CausalDiffusionInferencePipeline`) spends per step, at full size (Wan2.1-T2V-1.3B geometry,
480p latents 16 x 60 x 104, blocks of 3 frames, synthetic weights), two comparisons interleaved in one process:

  (a) the step glue: ONE ifx_cfg_unipc_step launch (`FlowUniPCSchedule.step_cfg`) against the same step as torch operators on the
      device — the guidance mix of the pipeline and the solver's update applied operator by operator in bf16, as upstream's
      `FlowUniPCMultistepScheduler.step` does (coefficients precomputed on the host here, so upstream's 0-dim tensor arithmetic and
      `linalg.solve` are NOT charged to it).  Device time per block of `--steps` steps from events, and the host time to enqueue it.
  (b) a block of `--steps` sampling steps + the clean-context re-run through the pipeline, `forward_cfg` (the two forwards of a step
      on two streams) against the two `forward` calls one after the other; wall time per block behind a device synchronise.

Every leg is run `--rounds` times in the order A B A B ...; the figures are the medians and the spread of the rounds.

    python tools/bench_causal_diffusion.py [--steps 50] [--rounds 5] [--layers 30] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BF = torch.bfloat16
WAN_1_3B = dict(patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=1536, ffn_dim=8960, freq_dim=256, text_dim=4096, out_dim=16,
                num_heads=12, num_layers=30, eps=1e-6)
B, NF, C, H, W = 1, 3, 16, 60, 104


def torch_step(c, guidance, fc, fu, x, last, m1, m2):
    """The step as torch operators on bf16 device tensors: every operator one launch and one rounding."""
    flow = fu + guidance * (fc - fu)
    m_t = x - c.sigma * flow
    x_c = x
    if c.use_corrector:
        x_c = c.c_last * last + c.c_m1 * m1
        if c.corrector_order == 2:
            x_c = x_c + c.c_d1 * (m2 - m1)
        x_c = x_c + c.c_dt * (m_t - m1)
    x_next = c.p_x * x_c + c.p_m * m_t
    if c.predictor_order == 2:
        x_next = x_next + c.p_d * (m1 - m_t)
    return x_next, x_c, m_t


def bench_glue(steps, rounds):
    from inferix_amd.schedulers import FlowUniPCSchedule
    g = torch.Generator(device="cuda").manual_seed(0)
    x0 = torch.randn(B, NF, C, H, W, device="cuda", generator=g).to(BF)
    # the flows in the model's layout: [B, C, F, H, W] viewed [B, F, C, H, W]
    fc = torch.randn(B, C, NF, H, W, device="cuda", generator=g).to(BF).permute(0, 2, 1, 3, 4)
    fu = torch.randn(B, C, NF, H, W, device="cuda", generator=g).to(BF).permute(0, 2, 1, 3, 4)
    s = FlowUniPCSchedule()
    s.set_timesteps(steps, shift=5.0)
    table, ts = s.coefficients(), s.timesteps.tolist()

    def fused():
        s.set_timesteps(steps, shift=5.0)
        x = x0
        for t in ts:
            x = s.step_cfg(fc, fu, 3.0, t, x)[0]
        return x

    def operators():
        x, last, m1, m2 = x0, None, None, None
        for c in table:
            x, last, m_t = torch_step(c, 3.0, fc, fu, x, last, m1, m2)
            m1, m2 = m_t, m1
        return x
    out = {}
    legs = {"fused": fused, "torch_operators": operators}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    res = {k: {"device_ms": [], "host_ms": []} for k in legs}
    finals = {}
    for _ in range(rounds):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            e0.record()
            finals[k] = f()
            e1.record()
            h1 = time.perf_counter()
            torch.cuda.synchronize()
            res[k]["device_ms"].append(e0.elapsed_time(e1))
            res[k]["host_ms"].append((h1 - h0) * 1e3)
    for k, r in res.items():
        out[k] = {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in r.items()}
    a, b = finals["fused"].double(), finals["torch_operators"].double()
    out["rel_l2_fused_vs_operators"] = float((a - b).norm() / b.norm())
    out["bytes_per_step_fused"] = 2 * 9 * B * NF * C * H * W
    return out


def bench_block(steps, rounds, layers):
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalDiffusionInferencePipeline
    from inferix_amd.wan import HipCausalWanModel, HipWanDiffusionWrapper
    from inferix_amd.wan.synthetic import synthetic_state_dict
    cfg = dict(WAN_1_3B, num_layers=layers)
    model = HipCausalWanModel(**cfg, device="cuda")
    model.load_state_dict(synthetic_state_dict(model, seed=0))
    gen = HipWanDiffusionWrapper(model=model, timestep_shift=5.0)
    g = torch.Generator().manual_seed(1)
    pe = {}
    for name, n in (("pos", 40), ("neg", 25)):
        e = torch.zeros(1, 512, 4096)
        e[:, :n] = torch.randn(1, n, 4096, generator=g)
        pe[name] = e.to(BF).cuda()
    enc = lambda text_prompts: {"prompt_embeds": pe["neg" if text_prompts[0] == "negative" else "pos"]}
    noise = torch.randn(B, NF, C, H, W, generator=g).to(BF).cuda()
    pipes, out = {}, {}
    for name, pair in (("paired", True), ("unpaired", False)):
        args = SimpleNamespace(num_train_timestep=1000, timestep_shift=5.0, guidance_scale=3.0, negative_prompt="negative",
                               num_frame_per_block=NF, independent_first_frame=False, frame_seq_length=1560,
                               kv_cache_tokens=NF * 1560, pair_forwards=pair)
        p = CausalDiffusionInferencePipeline(args, "cuda", generator=gen, text_encoder=enc, vae=None)
        p.sampling_steps = steps
        pipes[name] = (p, KVCacheManager("cuda"), KVCacheManager("cuda"), [KVCacheRequest(name)])

    def run(name):
        p, kp, kn, reqs = pipes[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat = p.inference(noise=noise, text_prompts=["a prompt"], kv_cache_manager_pos=kp, kv_cache_manager_neg=kn,
                          kv_cache_requests=reqs, decode_mode=DecodeMode.NO_DECODE)        # ends in check_device(sync=True)
        return (time.perf_counter() - t0) * 1e3, lat
    lats = {}
    for name in pipes:
        _, lats[name] = run(name)                       # warm-up: caches, code objects, scratch of both chains
    res = {k: [] for k in pipes}
    for _ in range(rounds):
        for name in pipes:
            ms, lat = run(name)
            res[name].append(ms)
            assert torch.equal(lat, lats[name])
    for k, v in res.items():
        out[k] = {"block_ms": {"median": statistics.median(v), "min": min(v), "max": max(v)},
                  "ms_per_step": statistics.median(v) / (steps + 1)}
    out["bit_identical"] = bool(torch.equal(lats["paired"], lats["unpaired"]))
    out["forwards_per_block"] = 2 * (steps + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_causal_diffusion needs an MI355X: there is nothing to time on the host")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "layers": a.layers,
           "latents": [B, NF, C, H, W], "glue": bench_glue(a.steps, a.rounds)}
    if not a.skip_block:
        res["block"] = bench_block(a.steps, a.rounds, a.layers)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""One MAGI core-attention forward on the 8-bit cache against the bf16 launches, per launch.

Legs, alternating in ONE process, medians of --reps after --warmup rounds, the 8-bit leg timed twice (A/A) for the spread:
  kv8      one ifx_attn_fwd_kv8_ranges launch for all ranges over the e4m3 cache
  bf16_each  today's core_attention: one bf16 launch per range
  bf16_ranges  ifx_attn_fwd_ranges, all ranges in one bf16 launch
Shape: --chunks denoising ranges of --chunk-tokens query rows; range i attends --prefix-chunks clean chunks plus chunks 0 .. i.  The
defaults are the rank shape of cp = 8 that dit.py's _range_attention was tuned on: 4 x 12150 queries x 3 heads on 1 kv head over
2 .. 5 chunks of keys.
`--clip`: the per-clip leg (clip_leg) instead.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inferix_amd import hip_ops as ops  # noqa: E402


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def clip_leg(a):
    """Per clip: tools/bench_magi_pipeline.py's real-model leg (MAGI-4.5B's dimensions, synthetic weights, --layers of them, the walk
    of config 5's latent) with the 8-bit cache off, on and off again (A/A), clips alternating; the latent rel-L2 between on and off."""
    import time
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench_magi_pipeline as P
    from inferix_amd.magi.schedule import ChunkSchedule
    from inferix_amd.magi.types import InferenceParams
    dev = torch.device("cuda")
    sch = ChunkSchedule(a.steps, P.WINDOW, P.CHUNKS, P.CW)
    models = {"bf16": P.real_model(a.layers, dev), "kv8": P.real_model(a.layers, dev, "fp8_e4m3")}
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.randn(1, P.C, P.CHUNKS * P.CW, P.H, P.W, device=dev, generator=g).repeat(2, 1, 1, 1, 1)
    y = torch.randn(2, P.CHUNKS, 800, 4096, device=dev, generator=g)
    masks = torch.zeros(2, P.CHUNKS, 800, device=dev)
    masks[0, :, :100] = 1
    masks[1, :, :2] = 1
    tokens = P.CW * (P.H // 2) * (P.W // 2)
    ms, finals, cache = {"bf16": [], "kv8": [], "bf16_again": []}, {}, {}
    for clip in range(a.clips + 1):
        for name in ms:
            model = models[name.split("_")[0]]
            x, ip = noise.clone(), InferenceParams(1, P.CHUNKS * tokens, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in sch.walk(model, x, y, masks, ip):
                pass
            torch.cuda.synchronize()
            if clip:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            finals[name] = x
            mgr = ip.kv_cache_manager
            cache[name] = sum(mgr.get_raw(ip.kv_cache_request, n).numel() * mgr.get_raw(ip.kv_cache_request, n).element_size()
                              for n in mgr.layers(ip.kv_cache_request))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rel = lambda p, q: float((p.float() - q.float()).norm() / q.float().norm())
    print(json.dumps({"leg": "clip", "layers": a.layers, "forwards_per_clip": sch.total_forward_step(), "clips": a.clips, "clip_ms_median": med,
                      "aa_spread": abs(med["bf16"] - med["bf16_again"]) / med["bf16"], "kv8_vs_bf16": med["bf16"] / med["kv8"],
                      "latent_rel_l2_kv8_vs_bf16": rel(finals["kv8"], finals["bf16"]),
                      "latent_rel_l2_bf16_again_vs_bf16": rel(finals["bf16_again"], finals["bf16"]), "cache_bytes": cache}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", action="store_true", help="the per-clip leg instead of the per-launch one")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--clips", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--heads", type=int, default=3)
    ap.add_argument("--kv-heads", type=int, default=1)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--chunk-tokens", type=int, default=12150)
    ap.add_argument("--prefix-chunks", type=int, default=1)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if a.clip:
        return clip_leg(a)
    hq, hk, ct, n = a.heads, a.kv_heads, a.chunk_tokens, a.chunks
    rows, keys = n * ct, (a.prefix_chunks + n) * ct
    q_ranges = [(i * ct, (i + 1) * ct) for i in range(n)]
    k_ranges = [(0, (a.prefix_chunks + i + 1) * ct) for i in range(n)]
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(rows, hq * 128, generator=g, device="cuda")
    k, v = (torch.randn(keys, hk, 128, generator=g, device="cuda") for _ in range(2))
    q_scale = ops.attn_q_prescale(128)[0]
    f8 = lambda t: t.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    q8, qb = f8(q * q_scale), (q * q_scale).bfloat16()
    view8 = ops.MagiKv8View(f8(k), f8(v), torch.ones(hk, device="cuda"))
    viewb = ops.KvCacheView(k.bfloat16(), v.bfloat16())
    out8, outb, outr = (torch.empty(rows, hq * 128, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    ln2 = 0.6931471805599453

    def bf16_each():
        for (qs, qe), (ks, ke) in zip(q_ranges, k_ranges):      # dit.py's _range_attention
            ops.attention_ld(qb[qs:qe], viewb, ke, outb[qs:qe], hq, kv_start=ks, scale=ln2, tag="attn_magi")

    legs = {"kv8": lambda: ops.attention_kv8_ranges(q8, view8, q_ranges, k_ranges, out8, hq),
            "bf16_each": bf16_each,
            "bf16_ranges": lambda: ops.attention_ranges(qb, viewb, q_ranges, k_ranges, outr, hq, scale=ln2),
            "kv8_again": lambda: ops.attention_kv8_ranges(q8, view8, q_ranges, k_ranges, out8, hq)}
    ms = {name: [] for name in legs}
    for r in range(a.warmup + a.reps):
        for name, fn in legs.items():
            t = timed(fn)
            if r >= a.warmup:
                ms[name].append(t)
    med = {name: statistics.median(v) for name, v in ms.items()}
    rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
    plan = ops.attention_kv8_ranges_plan(q_ranges, k_ranges, hq, hk)
    print(json.dumps({"shape": dict(heads=hq, kv_heads=hk, q_ranges=q_ranges, k_ranges=k_ranges), "median_ms": med,
                      "aa_spread": abs(med["kv8"] - med["kv8_again"]) / med["kv8"],
                      "kv8_vs_bf16_each": med["bf16_each"] / med["kv8"], "kv8_vs_bf16_ranges": med["bf16_ranges"] / med["kv8"],
                      "rel_l2_kv8_vs_bf16_each": rel(out8, outb), "rel_l2_bf16_ranges_vs_each": rel(outr, outb),
                      "grid": plan["grid"], "xcd_tiles": plan["xcd_tiles"], "xcd_cost": plan["xcd_cost"],
                      "cache_bytes": {"kv8": 2 * keys * hk * 128, "bf16": 4 * keys * hk * 128}}))


if __name__ == "__main__":
    main()

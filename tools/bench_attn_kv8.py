"""attention_kv8 (8-bit cache, FP8 MFMA) against the bf16 self-attention launch, alternating in one process:
4680 rows x 12 heads over 4680 / 14040 / 32760 keys, median and spread of N launches each, device events.
    python tools/bench_attn_kv8.py [--launches 24] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inferix_amd import hip_ops as ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, heads, hd = 4680, 12, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    qs, ln2 = ops.attn_q_prescale(hd)
    q = torch.randn(rows, heads, hd, device="cuda", generator=g)
    qb = (q * qs).to(torch.bfloat16)
    q8 = (q * qs).to(torch.float8_e4m3fn).view(torch.uint8)
    results = []
    for keys in (4680, 14040, 32760):
        k = torch.randn(keys, heads, hd, device="cuda", generator=g)
        v = torch.randn(keys, heads, hd, device="cuda", generator=g)
        kv16 = ops.KvCacheView(k.to(torch.bfloat16), v.to(torch.bfloat16))
        kv8 = ops.Kv8CacheView(k.to(torch.float8_e4m3fn).view(torch.uint8), (v / 4).to(torch.float8_e4m3fn).view(torch.uint8),
                               torch.full((heads,), 4.0, device="cuda"))
        o16, o8 = torch.empty_like(qb), torch.empty_like(qb)
        run = {"bf16": lambda: ops.attention(qb, kv16, keys, scale=ln2, out=o16, splits=1), "kv8": lambda: ops.attention_kv8(q8, kv8, keys, out=o8)}
        for f in run.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ev = {n: [] for n in run}
        for _ in range(a.launches):
            for n, f in run.items():          # alternating
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                ev[n].append((s, e))
        torch.cuda.synchronize()
        rec = {"rows": rows, "heads": heads, "keys": keys,
               "rel_l2_kv8_vs_bf16": float((o8.float() - o16.float()).norm() / o16.float().norm())}
        for n, pairs in ev.items():
            ms = sorted(s.elapsed_time(e) for s, e in pairs)
            rec[n] = {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "launches": len(ms),
                      "tflops": 4.0 * rows * keys * heads * hd / (statistics.median(ms) * 1e-3) / 1e12}
        print(json.dumps(rec))
        results.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

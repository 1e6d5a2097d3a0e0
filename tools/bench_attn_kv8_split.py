"""The split-key launch of the 8-bit self-attention against the unsplit launch, alternating in one process: rows x 12 heads over
4680 / 14040 / 32760 keys, legs `unsplit`, `split2`, `split3`, `auto` (what ifx_attn_kv8_split_plan picks), `unsplit_again` (the A/A
leg) and, for orientation, `bf16` (ops.attention with its own automatic split); medians of N launches each, device events.
    python tools/bench_attn_kv8_split.py [--launches 24] [--rows 1560 3120] [--out FILE.json]"""
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1560, 3120])
    ap.add_argument("--keys", type=int, nargs="+", default=[4680, 14040, 32760])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    heads, hd = 12, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    qs, ln2 = ops.attn_q_prescale(hd)
    results = []
    for rows in a.rows:
        q = torch.randn(rows, heads, hd, device="cuda", generator=g)
        qb, q8 = (q * qs).to(torch.bfloat16), (q * qs).to(torch.float8_e4m3fn).view(torch.uint8)
        for keys in a.keys:
            k, v = (torch.randn(keys, heads, hd, device="cuda", generator=g) for _ in range(2))
            kv16 = ops.KvCacheView(k.to(torch.bfloat16), v.to(torch.bfloat16))
            kv8 = ops.Kv8CacheView(k.to(torch.float8_e4m3fn).view(torch.uint8), (v / 4).to(torch.float8_e4m3fn).view(torch.uint8),
                                   torch.full((heads,), 4.0, device="cuda"))
            outs = {n: torch.empty_like(qb) for n in ("unsplit", "split2", "split3", "auto", "bf16")}
            kv8_leg = lambda n, s: (lambda: ops.attention_kv8(q8, kv8, keys, out=outs[n], splits=s))
            legs = {"unsplit": kv8_leg("unsplit", 1), "split2": kv8_leg("split2", 2), "split3": kv8_leg("split3", 3), "auto": kv8_leg("auto", None),
                    "unsplit_again": kv8_leg("unsplit", 1), "bf16": lambda: ops.attention(qb, kv16, keys, scale=ln2, out=outs["bf16"])}
            for f in legs.values():
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            ev = {n: [] for n in legs}
            for _ in range(a.launches):
                for n, f in legs.items():          # alternating
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    f()
                    e.record()
                    ev[n].append((s, e))
            torch.cuda.synchronize()
            ref = outs["unsplit"].float()
            rec = {"rows": rows, "heads": heads, "keys": keys, "auto_chunks": ops.attention_kv8_split_plan(rows, heads, 0, keys)["chunks"],
                   "bf16_splits": ops.attention_split_plan(rows, heads, keys),
                   "rel_l2_vs_unsplit": {n: float((outs[n].float() - ref).norm() / ref.norm()) for n in ("split2", "split3", "auto", "bf16")}}
            for n, pairs in ev.items():
                ms = sorted(s.elapsed_time(e) for s, e in pairs)
                rec[n] = {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1]}
            base = rec["unsplit"]["median_ms"]
            rec["aa_spread"] = abs(rec["unsplit_again"]["median_ms"] / base - 1.0)
            rec["vs_unsplit"] = {n: rec[n]["median_ms"] / base for n in ("split2", "split3", "auto", "bf16")}
            print(json.dumps(rec), flush=True)
            results.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""attention_kv8 (8-bit cache, FP8 MFMA) against the bf16 self-attention launch, alternating in one process:
4680 rows x 12 heads over 4680 / 14040 / 32760 keys, median and spread of N launches each, device events.
    python tools/bench_attn_kv8.py [--launches 24] [--out FILE.json]
`--multi`: INSTEAD, the multi-session launches of the 8-bit cache against the single launches back to back (8 items x 12 heads, legs
`singles`, `multi`, `singles_again` alternating, medians of N): the self-attention over key counts spread across 4680 .. 32760 with
4680-row items, the same with 1560-row items (a 1-frame forward) among them, and the append of 8 x 4680 rows."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inferix_amd import hip_ops as ops  # noqa: E402


MULTI_SETS = {"8 x 4680 rows": [(4680, k) for k in (18720, 4680, 28080, 9360, 32760, 14040, 23400, 14040)],
              "4 x 1560 + 4 x 4680 rows": [(1560, 1560), (4680, 28080), (1560, 1560), (4680, 9360), (1560, 14040), (4680, 32760), (1560, 1560), (4680, 18720)]}


def bench_multi(launches):
    heads, hd, cap = 12, 128, 32760
    g = torch.Generator(device="cuda").manual_seed(0)
    qs = ops.attn_q_prescale(hd)[0]
    byt = lambda *shape: torch.randn(*shape, device="cuda", generator=g).to(torch.float8_e4m3fn).view(torch.uint8)
    views = [ops.Kv8CacheView(byt(cap, heads, hd), byt(cap, heads, hd), torch.full((heads,), 4.0, device="cuda")) for _ in range(8)]
    results = []

    def race(name, singles, multi, extra):
        legs = dict(singles=singles, multi=multi, singles_again=singles)
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ev = {n: [] for n in legs}
        for _ in range(launches):
            for n, f in legs.items():          # alternating
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                ev[n].append((s, e))
        torch.cuda.synchronize()
        rec = dict(what=name, launches=launches, **extra)
        for n, pairs in ev.items():
            ms = sorted(s.elapsed_time(e) for s, e in pairs)
            rec[n] = {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1]}
        rec["aa_spread"] = abs(rec["singles_again"]["median_ms"] / rec["singles"]["median_ms"] - 1.0)
        rec["multi_vs_singles"] = rec["multi"]["median_ms"] / rec["singles"]["median_ms"]
        print(json.dumps(rec), flush=True)
        results.append(rec)
    for name, shape in MULTI_SETS.items():
        items = [((torch.randn(rows, heads, hd, device="cuda", generator=g) * qs).to(torch.float8_e4m3fn).view(torch.uint8), v, keys,
                  torch.empty(rows, heads, hd, dtype=torch.bfloat16, device="cuda")) for (rows, keys), v in zip(shape, views)]
        alone = [ops.attention_kv8(q8, v, keys).clone() for q8, v, keys, _ in items]
        plan = ops.attention_kv8_multi_plan([(r, 0, k) for r, k in shape], heads)
        race("attention, " + name, lambda: [ops.attention_kv8(q8, v, keys, out=o) for q8, v, keys, o in items],
             lambda: ops.attention_kv8_multi(items, heads),
             dict(items=shape, heads=heads, grid=plan["grid"], xcd_cost=plan["xcd_cost"], tflops_ops=sum(4.0 * r * k * heads * hd for r, k in shape)))
        assert all(torch.equal(o, a_) for (_, _, _, o), a_ in zip(items, alone)), "the multi launch differs from the single launches"
    rows, dim = 4680, heads * hd
    freqs = torch.view_as_real(torch.polar(torch.ones(1024, hd // 2, dtype=torch.float64), torch.rand(1024, hd // 2, dtype=torch.float64))).contiguous().cuda()
    wq, wk = (torch.ones(dim, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    qkv = torch.randn(8 * rows, 3 * dim, device="cuda", generator=g).to(torch.bfloat16)
    app = [(qkv[i * rows:(i + 1) * rows], ops.RopeGridSpec(freqs, 3 * i, 30, 52, q_scale=qs), v, 3 * rows, torch.empty(rows, dim, dtype=torch.uint8, device="cuda"))
           for i, v in enumerate(views)]
    race("append, 8 x 4680 rows", lambda: [ops.rmsnorm_rope_kv8_append(x, wq, wk, 1e-6, r, v, s0, dim, q_out=q) for x, r, v, s0, q in app],
         lambda: ops.rmsnorm_rope_kv8_append_multi(app, wq, wk, 1e-6, dim), dict(rows=rows, dim=dim, bytes_moved=9.0 * 8 * rows * dim))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.multi:
        results = bench_multi(a.launches)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
        return
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

"""The 8-bit ring cache (kv_cache_dtype='fp8_e4m3_ring') against what it replaces, legs alternating in one process, medians of N
launches by device events, every leg twice for the A/A spread.
  launch: 4680 rows x 12 heads over 14040 and 32760 keys in groups of 1560 — the grouped walk (ifx_attn_fwd_kv8_grouped) against the
          flat one (ifx_attn_fwd_kv8) on the same bytes (equal scales, so the outputs are compared too).
  block:  a layer's self-attention part at the streaming_steady shape (a window of 21 frames, 3 of them the sink, saturated; a block of
          3 frames evicts 3): the ring format (per-frame scales in torch ops, ring append, grouped attention) against the bf16 rolling
          path (shift kernel, append, bf16 attention).
  multi:  the launches of a ragged forward over ring caches (include/inferix_hip_kv8_ring_sessions.h) against the same samples one by
          one: `append` — 8 x 4680 rows, the fused launch (scales, V bytes, q, K) against per sample the torch calibration and the
          ring append, and the calibration alone; `attention` — one grouped multi launch against its single grouped launches, for
          8 x 4680 rows over 4680 .. 32760 keys and for a set with four 1-frame items.
  split:  1560 rows x 12 heads (a 1-frame forward: 84 workgroups unsplit) over 1 .. 21 frames of keys — the grouped split-key launch
          (ifx_attn_fwd_kv8_grouped_split) in 2 chunks, 3 chunks and the chunks its plan picks when any chunk size is allowed, against
          the unsplit grouped launch, and the flat split launch in 2 chunks on the same bytes for orientation.
    python tools/bench_attn_kv8_ring.py [--launches 24] [--multi-only | --split-only] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inferix_amd import hip_ops as ops  # noqa: E402
from inferix_amd.wan.components import rope_table  # noqa: E402

HEADS, HD, G, H, W = 12, 128, 1560, 30, 52
F8, BF = torch.float8_e4m3fn, torch.bfloat16


def timed(legs, launches):
    """Median / min / max ms of each leg, the legs alternating; `legs` maps a name to a callable."""
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ev = {n: [] for n in legs}
    for _ in range(launches):
        for n, f in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            ev[n].append((s, e))
    torch.cuda.synchronize()
    out = {}
    for n, pairs in ev.items():
        ms = sorted(s.elapsed_time(e) for s, e in pairs)
        out[n] = {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1]}
    return out


def bench_multi(launches):
    g = torch.Generator(device="cuda").manual_seed(1)
    qs, _ = ops.attn_q_prescale(HD)
    rows, dim, slots, out = 3 * G, HEADS * HD, 21 * G, []
    wq, wk = (torch.ones(dim, dtype=BF, device="cuda") for _ in range(2))
    ring = lambda: ops.Kv8RingView(*(torch.randn(slots, HEADS, HD, device="cuda", generator=g).to(F8).view(torch.uint8) for _ in range(2)),
                                   torch.full((slots // G, HEADS), 4.0, device="cuda"), G)
    samples = []          # sample i appends block i of its video (no sink, nothing evicted yet) and attends (i + 1) x 4680 keys
    for i in range(8):
        qkv = torch.randn(rows, 3 * dim, device="cuda", generator=g).to(BF)
        samples.append(dict(qkv=qkv, rope=ops.RopeGridSpec(rope_table(HD).cuda(), 3 * (i % 7), H, W, q_scale=qs), ring=ring(), start=(i % 7) * rows,
                            keys=(i % 7 + 1) * rows, q8=torch.empty(rows, dim, dtype=torch.uint8, device="cuda"),
                            o=torch.empty(rows, HEADS, HD, dtype=BF, device="cuda")))

    def calibrate(s):
        amax = s["qkv"][:, 2 * dim:].float().abs().view(3, G, HEADS, HD).amax(dim=(1, 3))
        s["ring"].v_scale[s["start"] // G:s["start"] // G + 3].copy_(torch.exp2(torch.ceil(torch.log2(amax.clamp_min(2.0 ** -20) / 448.0))))

    def per_sample():
        for s in samples:
            calibrate(s)
            ops.rmsnorm_rope_kv8_append_ring(s["qkv"], wq, wk, 1e-6, s["rope"], s["ring"], 0, slots, s["start"], dim, q_out=s["q8"])

    def calibration_only():
        for s in samples:
            calibrate(s)
    app = [(s["qkv"], s["rope"], s["ring"], 0, slots, s["start"], s["q8"]) for s in samples]
    fused = lambda: ops.rmsnorm_rope_kv8_append_ring_multi(app, wq, wk, 1e-6, dim)
    legs = {"per_sample": per_sample, "fused": fused, "calibration_only": calibration_only, "per_sample_again": per_sample, "fused_again": fused}
    rec = {"what": "multi append", "items": 8, "rows": rows, "heads": HEADS, "group_tokens": G, **timed(legs, launches)}
    rec["aa_spread"] = max(abs(rec[n + "_again"]["median_ms"] / rec[n]["median_ms"] - 1.0) for n in ("per_sample", "fused"))
    rec["fused_vs_per_sample"] = rec["fused"]["median_ms"] / rec["per_sample"]["median_ms"]
    rec["calibration_share_of_per_sample"] = rec["calibration_only"]["median_ms"] / rec["per_sample"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
    one_frame = [dict(s, q8=s["q8"][:G], o=s["o"][:G]) for s in samples[:4]]
    for name, group in (("8 x 4680 rows", samples), ("4 x 1560 rows", one_frame), ("4 x 4680 + 4 x 1560 rows", samples[:4] + one_frame)):
        att = [(s["q8"].view(-1, HEADS, HD), s["ring"], s["keys"], s["o"]) for s in group]

        def singles():
            for q8, view, keys, o in att:
                ops.attention_kv8_grouped(q8, view, keys, out=o)
        multi = lambda: ops.attention_kv8_grouped_multi(att, HEADS)
        legs = {"singles": singles, "multi": multi, "singles_again": singles, "multi_again": multi}
        rec = {"what": "multi attention", "set": name, "rows": [a_[0].shape[0] for a_ in att], "keys": [a_[2] for a_ in att], "heads": HEADS,
               "group_tokens": G, **timed(legs, launches)}
        rec["aa_spread"] = max(abs(rec[n + "_again"]["median_ms"] / rec[n]["median_ms"] - 1.0) for n in ("singles", "multi"))
        rec["multi_vs_singles"] = rec["multi"]["median_ms"] / rec["singles"]["median_ms"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def bench_split(launches, frames=(1, 2, 3, 4, 5, 6, 9, 21)):
    g = torch.Generator(device="cuda").manual_seed(2)
    qs, _ = ops.attn_q_prescale(HD)
    q8 = (torch.randn(G, HEADS, HD, device="cuda", generator=g) * qs).to(F8).view(torch.uint8)
    out = []
    for keys in (f * G for f in frames):
        k8, v8 = (torch.randn(keys, HEADS, HD, device="cuda", generator=g).to(F8).view(torch.uint8) for _ in range(2))
        flat = ops.Kv8CacheView(k8, v8, torch.full((HEADS,), 4.0, device="cuda"))
        ring = ops.Kv8RingView(k8, v8, torch.full((keys // G, HEADS), 4.0, device="cuda"), G)
        with ops.option_scope("attn_kv8_grouped_split_min_tiles", 1):
            pick = ops.attention_kv8_grouped_split_plan(G, HEADS, G, keys)
        o = {n: torch.empty(G, HEADS, HD, dtype=BF, device="cuda") for n in ("unsplit", "split")}
        grouped = lambda n, name="split": (lambda: ops.attention_kv8_grouped(q8, ring, keys, out=o[name], splits=n))
        legs = {"unsplit": grouped(1, "unsplit"), "split2": grouped(2), "split3": grouped(3), "pick": grouped(pick["chunks"]),
                "flat_split2": lambda: ops.attention_kv8(q8, flat, keys, out=o["split"], splits=2)}
        legs.update(unsplit_again=legs["unsplit"], pick_again=legs["pick"])
        rec = {"what": "split", "rows": G, "heads": HEADS, "keys": keys, "group_tokens": G, "key_tiles": pick["key_tiles"],
               "pick_chunks": pick["chunks"], "pick_tiles_per_chunk": pick["tiles_per_chunk"], **timed(legs, launches)}
        legs["pick"]()
        rec["rel_l2_pick_vs_unsplit"] = float((o["split"].float() - o["unsplit"].float()).norm() / o["unsplit"].float().norm())
        rec["aa_spread"] = max(abs(rec[n + "_again"]["median_ms"] / rec[n]["median_ms"] - 1.0) for n in ("unsplit", "pick"))
        for n in ("split2", "split3", "pick", "flat_split2"):
            rec[n + "_vs_unsplit"] = rec[n]["median_ms"] / rec["unsplit"]["median_ms"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--split-only", action="store_true", help="the `split` section alone")
    ap.add_argument("--multi-only", action="store_true", help="the `multi` section alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.multi_only or a.split_only:
        results = bench_multi(a.launches) if a.multi_only else bench_split(a.launches)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
        return
    g = torch.Generator(device="cuda").manual_seed(0)
    qs, ln2 = ops.attn_q_prescale(HD)
    rows, dim, results = 3 * G, HEADS * HD, []
    q = torch.randn(rows, HEADS, HD, device="cuda", generator=g)
    q8 = (q * qs).to(F8).view(torch.uint8)
    # ---- per launch
    for keys in (9 * G, 21 * G):
        k, v = (torch.randn(keys, HEADS, HD, device="cuda", generator=g) for _ in range(2))
        k8, v8 = k.to(F8).view(torch.uint8), (v / 4).to(F8).view(torch.uint8)
        flat = ops.Kv8CacheView(k8, v8, torch.full((HEADS,), 4.0, device="cuda"))
        ring = ops.Kv8RingView(k8, v8, torch.full((keys // G, HEADS), 4.0, device="cuda"), G)
        outs = {n: torch.empty(rows, HEADS, HD, dtype=BF, device="cuda") for n in ("flat", "grouped")}
        legs = {"flat": lambda: ops.attention_kv8(q8, flat, keys, out=outs["flat"]),
                "grouped": lambda: ops.attention_kv8_grouped(q8, ring, keys, out=outs["grouped"])}
        legs.update(flat_again=legs["flat"], grouped_again=legs["grouped"])
        rec = {"what": "launch", "rows": rows, "heads": HEADS, "keys": keys, "group_tokens": G,
               "key_tiles": {"flat": ops.attention_kv8_plan(rows, HEADS, 0, keys)["key_tiles"],
                             "grouped": ops.attention_kv8_grouped_plan(rows, HEADS, G, keys)["key_tiles"]}, **timed(legs, a.launches)}
        rec["rel_l2_grouped_vs_flat"] = float((outs["grouped"].float() - outs["flat"].float()).norm() / outs["flat"].float().norm())
        rec["aa_spread"] = max(abs(rec[n + "_again"]["median_ms"] / rec[n]["median_ms"] - 1.0) for n in ("flat", "grouped"))
        rec["grouped_vs_flat"] = rec["grouped"]["median_ms"] / rec["flat"]["median_ms"]
        print(json.dumps(rec), flush=True)
        results.append(rec)
    # ---- per block, the window saturated: sink 3 frames, ring 18, a block of 3 frames evicts 3
    slots, sink = 21 * G, 3 * G
    qkv = torch.randn(rows, 3 * dim, device="cuda", generator=g).to(BF)
    wq, wk = (torch.ones(dim, dtype=BF, device="cuda") for _ in range(2))
    rope = ops.RopeGridSpec(rope_table(HD).cuda(), 21, H, W, q_scale=qs)
    kv16 = ops.KvCacheView(*(torch.randn(slots, HEADS, HD, device="cuda", generator=g).to(BF) for _ in range(2)))
    ring = ops.Kv8RingView(kv16.k.to(F8).view(torch.uint8), (kv16.v / 4).to(F8).view(torch.uint8),
                           torch.full((slots // G, HEADS), 4.0, device="cuda"), G)
    scratch = torch.empty((slots - sink - rows) * dim, dtype=BF, device="cuda")
    qb, q8b = torch.empty(rows, dim, dtype=BF, device="cuda"), torch.empty(rows, dim, dtype=torch.uint8, device="cuda")
    ob = torch.empty(rows, HEADS, HD, dtype=BF, device="cuda")
    turn = [0]

    def bf16_block():
        ops.kv_roll(kv16, sink, rows, slots - sink - rows, scratch)
        ops.rmsnorm_rope_kv_append(qkv, wq, wk, 1e-6, rope, kv16, slots - rows, dim, q_out=qb)
        ops.attention(qb.view(rows, HEADS, HD), kv16, slots, scale=ln2, out=ob)

    def ring_block():
        turn[0] = (turn[0] + rows) % (slots - sink)          # the eviction: the ring's offset advances, nothing moves
        start = slots - rows + turn[0]
        amax = qkv[:, 2 * dim:].float().abs().view(3, G, HEADS, HD).amax(dim=(1, 3))
        g0 = (sink + (start - sink) % (slots - sink)) // G   # (a block of 3 frames on a ring of 18 never straddles the ring's end)
        ring.v_scale[g0:g0 + 3].copy_(torch.exp2(torch.ceil(torch.log2(amax.clamp_min(2.0 ** -20) / 448.0))))
        ops.rmsnorm_rope_kv8_append_ring(qkv, wq, wk, 1e-6, rope, ring, sink, slots - sink, start, dim, q_out=q8b)
        ops.attention_kv8_grouped(q8b.view(rows, HEADS, HD), ring, slots, out=ob)
    legs = {"bf16_roll": bf16_block, "fp8_ring": ring_block, "bf16_roll_again": bf16_block, "fp8_ring_again": ring_block}
    rec = {"what": "block", "rows": rows, "heads": HEADS, "window": slots, "sink": sink, **timed(legs, a.launches)}
    rec["aa_spread"] = max(abs(rec[n + "_again"]["median_ms"] / rec[n]["median_ms"] - 1.0) for n in ("bf16_roll", "fp8_ring"))
    rec["ring_vs_bf16"] = rec["fp8_ring"]["median_ms"] / rec["bf16_roll"]["median_ms"]
    print(json.dumps(rec), flush=True)
    results.append(rec)
    results += bench_multi(a.launches)
    results += bench_split(a.launches)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GPU: the two matrix-instruction forms of the self-attention loop (option attn_mfma 1 = 32x32x16, 2 = 16x16x32) per launch, on random
data, alternating in one process on one device.  N = 4680 queries x 12 heads (one 480p chunk of three frames) against L keys, q prescaled
(the exponent form the model runs), unsplit, contiguous cache and (--paged) pages of 1560 keys.
Prints per (L, view) the median and min wall time of each form over the rounds (one round = `--reps` launches between two events).
usage: tools/bench_attn_mfma.py [--rounds 7] [--reps 10] [--lengths 4680,18720,32760] [--paged] [--only FORM --length L: one form, for counter passes]"""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lengths", default="4680,18720,32760")
    ap.add_argument("--paged", action="store_true")
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    rows, heads, hd = 4680, 12, 128
    g = torch.Generator().manual_seed(7)
    q_scale, scale = ops.attn_q_prescale(hd)
    q = (torch.randn(rows, heads, hd, generator=g) * q_scale).to(torch.bfloat16).cuda()
    out = torch.empty_like(q)
    res = []
    for L in [int(x) for x in a.lengths.split(",")]:
        k = torch.randn(L, heads, hd, generator=g).to(torch.bfloat16).cuda()
        v = torch.randn(L, heads, hd, generator=g).to(torch.bfloat16).cuda()
        views = {"contiguous": ops.KvCacheView(k, v)}
        if a.paged:
            ps = 1560
            views["paged"] = ops.KvCacheView(k, v, torch.arange(L // ps, dtype=torch.int32).flip(0).contiguous().cuda(), ps)
        for name, view in views.items():
            times = {1: [], 2: []}
            forms = (a.only,) if a.only else (1, 2)
            for rnd in range(a.rounds + 1):                 # round 0 warms both forms up
                for form in forms:
                    ops.set_option("attn_mfma", form)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        ops.attention(q, view, L, scale=scale, out=out, splits=1)
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        times[form].append(e0.elapsed_time(e1) * 1e3 / a.reps)
            ops.set_option("attn_mfma", 0)
            row = {"L": L, "view": name}
            for form in forms:
                t = times[form]
                row[f"form{form}_us_median"] = round(statistics.median(t), 1)
                row[f"form{form}_us_min"] = round(min(t), 1)
                row[f"form{form}_tflops_median"] = round(4.0 * rows * L * heads * hd / statistics.median(t) / 1e6, 1)
            if not a.only:
                row["form2_median_beats_form1_min"] = row["form2_us_median"] < row["form1_us_min"]
            res.append(row)
            print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times MAGI-1's caption encoder (T5 v1.1 XXL, fp32: d_model 4096, 64 heads, d_ff 10240, 24 layers, synthetic weights) at the padded
length of 800 on one MI355X:

* ms per prompt of `HipT5v11Encoder` with rows="all", and with rows="valid" at 120 valid tokens;
* the comparison: the same encoder as plain fp32 torch ops on the device (`tests/magi_t5_util.encoder_forward`, the restatement the
  parity tests use), A/B interleaved in one process, medians over the rounds after warm-ups;
* per kernel, at the encoder's shapes: time, and TFLOP/s against the 157 TFLOP/s fp32 matrix peak;
* the distance between the two results (both are fp32 evaluations of one formula).

Needs a GPU: there is no CPU path.  usage:  python tools/bench_magi_t5.py [--rounds 7] [--layers 24] [--out result.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_F32_TFLOPS = 157.0


def timed(fn, reps: int) -> float:
    """Median ms of `fn` over `reps` runs, each between device events and a synchronise."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--length", type=int, default=800)
    ap.add_argument("--valid", type=int, default=120)
    ap.add_argument("--parity", action="store_true", help="per-block distances of both fp32 evaluations from a float64 one (38 GB more)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_magi_t5: no GPU visible; timings are taken on an MI355X only")
    import magi_t5_util as U
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.t5 import HipT5v11Encoder

    torch.backends.cuda.matmul.allow_tf32 = False
    L, d, heads, ff = args.length, 4096, 64, 10240
    enc = HipT5v11Encoder(None, d_model=d, num_heads=heads, d_ff=ff, num_layers=args.layers, device="cuda")
    enc.load_synthetic(0)
    case = U.T5Case(d_model=d, num_heads=heads, d_ff=ff, num_layers=args.layers, L=L, lens=(L,), seed=0, vocab=32128)
    sd = {"shared.weight": enc.emb, "encoder.final_layer_norm.weight": enc.final_norm,
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": enc.rel_bias}
    for i, b in enumerate(enc.blocks):      # views of the fused weights: nothing is copied
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        for j, n in enumerate("qkv"):
            sd[a + f"SelfAttention.{n}.weight"] = b["wqkv"][j * d:(j + 1) * d]
        sd.update({a + "SelfAttention.o.weight": b["wo"], a + "layer_norm.weight": b["norm1"], f + "layer_norm.weight": b["norm2"],
                   f + "DenseReluDense.wi_0.weight": b["wi"][:ff], f + "DenseReluDense.wi_1.weight": b["wi"][ff:],
                   f + "DenseReluDense.wo.weight": b["wo_ff"]})
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(2, 32128, (1, L), generator=g)
    full = torch.ones(1, L, dtype=torch.int64)
    short = torch.zeros(1, L, dtype=torch.int64)
    short[:, :args.valid] = 1
    ids_d, full_d, short_d = ids.cuda(), full.cuda(), short.cuda()

    arms = {
        "hip_all": lambda: enc(ids, full, rows="all"),
        "torch_fp32": lambda: U.encoder_forward(sd, case, ids_d, full_d),
        f"hip_valid_{args.valid}": lambda: enc(ids, short, rows="valid"),
        f"hip_all_{args.valid}": lambda: enc(ids, short, rows="all"),
        f"torch_fp32_{args.valid}": lambda: U.encoder_forward(sd, case, ids_d, short_d),
    }
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):          # interleaved: every round runs every arm once
            for k, fn in arms.items():
                times[k].append(timed(fn, 1))
        hip, ref = arms["hip_all"](), arms["torch_fp32"]()
        keep = short_d.gt(0)
        hv, rv = arms[f"hip_valid_{args.valid}"](), arms[f"torch_fp32_{args.valid}"]()
    result = {"layers": args.layers, "length": L, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "ms_per_prompt": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
              "rel_l2_hip_vs_torch_fp32": {"all": U.rel_l2(hip, ref), f"valid_{args.valid}": U.rel_l2(hv[keep], rv[keep])}}
    if args.parity:
        # block by block at full width, against the float64 evaluation of the same weights: where the two fp32 evaluations stand, and
        # how fast a last-bit difference grows through blocks of random weights with peaked softmaxes
        with torch.no_grad():
            t_hip, t_32, t_64 = [], [], []
            enc(ids, full, rows="all", taps=t_hip)
            U.encoder_forward(sd, case, ids_d, full_d, t_32)
            U.encoder_forward({k: v.double() for k, v in sd.items()}, case, ids_d, full_d, t_64)
        result["parity_per_block"] = [{"block": i, "hip_vs_exact64": U.rel_l2(a, c), "torch_fp32_vs_exact64": U.rel_l2(b, c),
                                       "hip_vs_torch_fp32": U.rel_l2(a, b)} for i, (a, b, c) in enumerate(zip(t_hip, t_32, t_64))]
        del t_hip, t_32, t_64
    flops_layer = lambda m: 2.0 * m * d * (3 * d + d + 2 * ff + ff)
    flops_all = args.layers * (flops_layer(L) + 4.0 * heads * L * L * 64)
    result["encoder_tflops_hip_all"] = flops_all / (result["ms_per_prompt"]["hip_all"]["median"] * 1e-3) / 1e12

    # per kernel, at the encoder's shapes
    kern = {}
    r = lambda *s: torch.randn(*s, device="cuda")
    for M in (L, args.valid):
        x, h = r(M, d), r(M, ff)
        for name, inp, w in (("qkv", x, enc.blocks[0]["wqkv"]), ("o", x, enc.blocks[0]["wo"]), ("wi", x, enc.blocks[0]["wi"]),
                             ("wo", h, enc.blocks[0]["wo_ff"])):
            N, K = w.shape
            out = torch.empty(M, N, device="cuda")
            fn = lambda: ops.gemm_f32(inp, w, out=out)
            timed(fn, 3)
            ms = timed(fn, 15)
            kern[f"gemm_{name}_{M}x{N}x{K}"] = {"ms": ms, "tflops": 2.0 * M * N * K / (ms * 1e-3) / 1e12}
        gu = r(M, 2 * ff)
        for name, fn, fl in (("rmsnorm", lambda: ops.rmsnorm_f32(x, enc.final_norm, 1e-6), 3.0 * M * d),
                             ("gated_gelu", lambda: ops.t5_gated_gelu_f32(gu), 10.0 * M * ff)):
            timed(fn, 3)
            ms = timed(fn, 15)
            kern[f"{name}_{M}"] = {"ms": ms, "tflops": fl / (ms * 1e-3) / 1e12}
    qkv = r(L, 3 * d)
    qkv[:, :d] *= 0.5
    table = enc._bias_table(L)
    for n, mode in ((L, False), (args.valid, True), (args.valid, False)):
        seq = torch.tensor([n], dtype=torch.int32, device="cuda")
        fn = lambda: ops.t5_attention_f32(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], table, seq, 1, heads, valid_rows_only=mode)
        timed(fn, 3)
        ms = timed(fn, 15)
        rows = n if mode else L
        kern[f"attention_L{L}_keys{n}_{'valid' if mode else 'all'}_rows"] = {"ms": ms, "tflops": 4.0 * heads * rows * n * 64 / (ms * 1e-3) / 1e12}
    for v in kern.values():
        v["share_of_f32_peak"] = v["tflops"] / PEAK_F32_TFLOPS
    result["kernels"] = kern
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

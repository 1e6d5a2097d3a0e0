"""MAGI-1 ViT-VAE decoder, one tile on one MI355X: the published geometry (24 blocks of width 1024, 16 heads of 64 channels, patch
8 x 8 x 4, ln_in_attn, final projection; 4 x 32 x 32 latents + class token = 4097 tokens -> 16 x 256 x 256 pixels), synthetic weights
generated on the device.  Reports ms per tile decode through HipViTDecoder, ms and TFLOP/s of ifx_vit_attention alone
(4 tokens^2 64 heads FLOP), the per-kernel shares of a decode, and — the baseline, since nothing decoded a MAGI tile before — the same
tile through a plain torch evaluation of the restated module on the device (tests/magi_vit_util.py: nn.functional operators,
scaled_dot_product_attention, bf16).  The two are timed in alternating repetitions; min / median / max over the repetitions are printed.
    python tools/bench_magi_vae.py [--reps 7] [--iters 3] [--depth 24]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out


def spread(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--z-chans", type=int, default=16)
    a = ap.parse_args()
    import magi_vit_util as U
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.vae import HipViTDecoder
    assert torch.cuda.is_available(), "needs the GPU"
    cfg = U.VitConfig(video_size=256, video_length=16, patch_size=8, patch_length=4, z_chans=a.z_chans, embed_dim=1024, depth=a.depth,
                      num_heads=16, qkv_bias=True, ln_in_attn=True, use_final_proj=True)
    dec = HipViTDecoder(**cfg.ctor_kwargs(), device="cuda")
    dec.load_synthetic(seed=0)
    W = dec.state_dict()
    x = torch.randn(1, a.z_chans, *cfg.latent, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.bfloat16)
    tokens, heads = cfg.latent[0] * cfg.latent[1] * cfg.latent[2] + 1, cfg.num_heads
    qkv = torch.randn(tokens, 3 * 1024, device="cuda").to(torch.bfloat16)

    hip = lambda: dec(x)
    with torch.no_grad():
        ref = lambda: U.decoder_forward(W, cfg, x)
        attn = lambda: ops.vit_attention(qkv[:, :1024], qkv[:, 1024:2048], qkv[:, 2048:], batch=1, heads=heads)
        for f in (hip, ref, attn):           # warm-up: code objects, library algorithm choices
            f()
            f()
        t_hip, t_ref, t_attn = [], [], []
        for _ in range(a.reps):              # alternating repetitions: both see the same box at the same time
            ms, out_hip = timed(hip, a.iters)
            t_hip.append(ms)
            ms, out_ref = timed(ref, a.iters)
            t_ref.append(ms)
            ms, _ = timed(attn, 10 * a.iters)
            t_attn.append(ms)
    rel = float((out_hip.double() - out_ref.double()).norm() / out_ref.double().norm())
    attn_flop = 4.0 * tokens * tokens * 64 * heads
    res = {"workload": f"MAGI ViT-VAE decoder tile, {a.depth} blocks x 1024, 16 heads x 64, {tokens} tokens -> {tuple(out_hip.shape)}, bf16, synthetic weights",
           "hip_ms_per_tile": spread(t_hip), "torch_ms_per_tile": spread(t_ref),
           "hip_over_torch": round(statistics.median(t_hip) / statistics.median(t_ref), 3),
           "vit_attention_ms": spread(t_attn), "vit_attention_tflops": round(attn_flop / statistics.median(t_attn) / 1e9, 1),
           "hip_vs_torch_rel_l2": round(rel, 5), "finite": bool(torch.isfinite(out_hip.float()).all())}
    names = ("gemm", "layernorm", "vit_head_prep", "vit_attention", "vit_unpatch_conv")
    t = ops.KernelTimer(names=names)
    ops.set_kernel_timer(t)
    hip()
    ops.set_kernel_timer(None)
    summ = t.summary()
    total = sum(d["ms"] for d in summ.values())
    res["kernels"] = {k: {"launches": d["launches"], "ms": round(d["ms"], 3), "share": round(d["ms"] / total, 3),
                          "TFLOP/s": round(d["flops"] / d["ms"] / 1e9, 1) if d["flops"] else None} for k, d in summ.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

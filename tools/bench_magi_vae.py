"""MAGI-1 ViT-VAE decoder, one tile on one MI355X: the published geometry (24 blocks of width 1024, 16 heads of 64 channels, patch
8 x 8 x 4, ln_in_attn, final projection; 4 x 32 x 32 latents + class token = 4097 tokens -> 16 x 256 x 256 pixels), synthetic weights
generated on the device.  Reports ms per tile decode through HipViTDecoder, ms and TFLOP/s of ifx_vit_attention alone
(4 tokens^2 64 heads FLOP), the per-kernel shares of a decode, and — the baseline, since nothing decoded a MAGI tile before — the same
tile through a plain torch evaluation of the restated module on the device (tests/magi_vit_util.py: nn.functional operators,
scaled_dot_product_attention, bf16).  The two are timed in alternating repetitions; min / median / max over the repetitions are printed.
    python tools/bench_magi_vae.py [--reps 7] [--iters 3] [--depth 24]

--chunk: one config-5 chunk instead (1 x 16 x 6 x 90 x 90 latents, tiles of 12 x 256 x 256 pixels with the default overlap -> 24 frames of
720 x 720, uint8), two ways in alternating repetitions:
  (A) what a caller had before `tiled_decode_3d`: the reference's tile loop on the device — `vae.decode` per tile, each blend one torch
      statement per row / column / frame as `TileProcessor.blend_{t,v,h}` writes them, crop, concatenation, the uint8 operators;
  (B) `HipMagiVAEDecoder.tiled_decode_3d(..., uint8_output=True)`.
Prints ms per chunk for both and the ratio, whether the two results are identical, the per-kernel shares of (B), and for
ifx_vit_tile_blend its time against the bytes the plan implies (output bytes written + one read per own pixel and per active blend) at
8 TB/s.
    python tools/bench_magi_vae.py --chunk [--reps 5] [--depth 24]

--encode: the ENCODER on one 12 x 256 x 256-pixel tile (3 x 32 x 32 latents + class token = 3073 tokens) through HipViTEncoder against
the restated module in torch on the device (tests/magi_vit_encoder_util.py), alternating repetitions; the per-kernel shares of a tile and,
for the two new row kernels, their time against the bytes they move.
    python tools/bench_magi_vae.py --encode [--reps 7] [--iters 3] [--depth 24]

--encode-clip: `encode_prefix_video` of a 32-frame 720 x 1280 uint8 clip at fps 24 (3 x 4 x 7 tiles of 12 frames), two ways in
alternating repetitions:
  (A) the tile-by-tile loop over the same HIP encoder: `vae.encode` per tile (84 batch-1 forwards), the reference's in-place blend
      chain as eager torch statements, crop, concatenation;
  (B) `encode_prefix_video` (shape-batched tiles, the head kernel writing the arena, ifx_vit_latent_blend).
    python tools/bench_magi_vae.py --encode-clip [--reps 5] [--depth 24]"""
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


def blend_rows(a, b, dim, extent):
    """One blend of the reference's tile loop as eager torch: a statement per position along `dim`, Python-float weights."""
    extent = min(a.shape[dim], b.shape[dim], extent)
    for p in range(extent):
        b.select(dim, p).copy_(a.select(dim, a.shape[dim] - extent + p) * (1 - p / extent) + b.select(dim, p) * (p / extent))
    return b


def chunk_tile_by_tile(vae, z, plan):
    """(A): decode every tile, blend clones against the raw neighbours (temporal, upper, left), crop, concatenate, convert."""
    at, ah, aw = plan.axes
    raw = {}
    for idx in plan.tiles:
        (t0, t1), (h0, h1), (w0, w1) = plan.latent_span(idx)
        raw[idx] = vae.decode(z[:, :, t0:t1, h0:h1, w0:w1])
    frames = []
    for it in range(at.count):
        rows = []
        for ih in range(ah.count):
            row = []
            for iw in range(aw.count):
                tile = raw[it, ih, iw].clone()
                if it > 0:
                    tile = blend_rows(raw[it - 1, ih, iw], tile, 2, at.blend)
                if ih > 0:
                    tile = blend_rows(raw[it, ih - 1, iw], tile, 3, ah.blend)
                if iw > 0:
                    tile = blend_rows(raw[it, ih, iw - 1], tile, 4, aw.blend)
                row.append(tile[:, :, :at.limit, :ah.limit, :aw.limit])
            rows.append(torch.cat(row, dim=4))
        frames.append(torch.cat(rows, dim=3))
    x = torch.cat(frames, dim=2)
    N, C, T, H, W = x.shape
    x = x.permute(0, 2, 1, 3, 4).reshape(N * T, C, H, W)
    return ((x * 127.5) + 127.5).clamp(0, 255).type(torch.uint8)


def bench_chunk(a):
    import magi_vit_util as U
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    cfg = U.VitConfig(video_size=256, video_length=16, patch_size=8, patch_length=4, z_chans=a.z_chans, embed_dim=1024, depth=a.depth,
                      num_heads=16, qkv_bias=True, ln_in_attn=True, use_final_proj=True)
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda")
    vae.decoder.load_synthetic(seed=0)
    z = torch.randn(1, a.z_chans, 6, 90, 90, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.bfloat16)
    kw = dict(tile_sample_min_length=12, tile_sample_min_height=256, tile_sample_min_width=256, allow_spatial_tiling=True)
    plan = vae.tile_plan(z.shape, **kw)
    loop = lambda: chunk_tile_by_tile(vae, z, plan)
    hip = lambda: vae.tiled_decode_3d(z, uint8_output=True, **kw)
    with torch.no_grad():
        for f in (loop, hip):
            f()
        t_loop, t_hip = [], []
        for _ in range(a.reps):
            ms, out_loop = timed(loop, 1)
            t_loop.append(ms)
            ms, out_hip = timed(hip, 1)
            t_hip.append(ms)
    groups = {"x".join(map(str, k)): len(v) for k, v in plan.groups().items()}
    res = {"workload": f"MAGI config-5 chunk decode, {a.depth} blocks x 1024, z {tuple(z.shape)} -> uint8 {tuple(out_hip.shape)}, "
                       f"{len(plan.tiles)} tiles in groups {groups}, synthetic weights",
           "tile_by_tile_ms_per_chunk": spread(t_loop), "tiled_decode_3d_ms_per_chunk": spread(t_hip),
           "tiled_over_tile_by_tile": round(statistics.median(t_hip) / statistics.median(t_loop), 3),
           "identical": bool(torch.equal(out_loop, out_hip)),
           "differing_values": int((out_loop != out_hip).sum())}
    names = ("gemm", "layernorm", "vit_head_prep", "vit_attention", "vit_unpatch_conv", "vit_tile_blend")
    t = ops.KernelTimer(names=names)
    ops.set_kernel_timer(t)
    hip()
    ops.set_kernel_timer(None)
    summ = t.summary()
    total = sum(d["ms"] for d in summ.values())
    res["kernels"] = {k: {"launches": d["launches"], "ms": round(d["ms"], 3), "share": round(d["ms"] / total, 4)} for k, d in summ.items()}
    pixels, reads = plan.traffic_elements(z.shape[0])
    nbytes = pixels * 1 + reads * 2
    blend_ms = summ["vit_tile_blend"]["ms"]
    res["tile_blend"] = {"ms": round(blend_ms, 4), "bytes": nbytes, "ms_at_8TBps": round(nbytes / 8e12 * 1e3, 4),
                         "TB_per_s": round(nbytes / blend_ms / 1e9, 3)}
    # the same launch alone, back to back on the plan's own arena (the arena, 151 MB, does not fit the 256 MB cache next to the outputs'
    # write traffic, but a repeated launch may still find part of it there: the in-chunk figure above is the cold one)
    cp = next(iter(vae._tile_cache.values()))
    u8 = torch.empty_like(out_hip)
    bf = torch.empty(z.shape[0], 3, *plan.out_shape, dtype=torch.bfloat16, device="cuda")
    for key, kwargs, wr in (("uint8", dict(out=False, out_u8=u8), 1), ("bf16", dict(out=bf, out_u8=False), 2)):
        ms, _ = timed(lambda: ops.vit_tile_blend(cp.arena, cp.desc, cp.table, **kwargs), 20)
        by = pixels * wr + reads * 2
        res["tile_blend"]["alone_" + key] = {"ms": round(ms, 4), "bytes": by, "TB_per_s": round(by / ms / 1e9, 3)}
    print(json.dumps(res))


def published_encoder_config(a):
    import magi_vit_encoder_util as E
    return E.EncConfig(video_size=256, video_length=16, patch_size=8, patch_length=4, z_chans=a.z_chans, embed_dim=1024, depth=a.depth,
                       num_heads=16, qkv_bias=True, ln_in_attn=True, use_final_proj=True)


def kernel_shares(ops, fn, names):
    t = ops.KernelTimer(names=names)
    ops.set_kernel_timer(t)
    fn()
    ops.set_kernel_timer(None)
    summ = t.summary()
    total = sum(d["ms"] for d in summ.values())
    return {k: {"launches": d["launches"], "ms": round(d["ms"], 4), "share": round(d["ms"] / total, 4),
                "TB_per_s": round(d["bytes"] / d["ms"] / 1e9, 3) if d["bytes"] else None} for k, d in summ.items()}


def bench_encode_tile(a):
    import magi_vit_encoder_util as E
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.vae import HipViTEncoder
    cfg = published_encoder_config(a)
    enc = HipViTEncoder(**cfg.ctor_kwargs(), device="cuda")
    enc.load_synthetic(seed=1)
    W = enc.state_dict()
    x = (torch.randn(1, 3, 12, 256, 256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 0.5).clamp(-1, 1).to(torch.bfloat16)
    hip = lambda: enc(x)
    with torch.no_grad():
        ref = lambda: E.encoder_forward(W, cfg, x)
        for f in (hip, ref):
            f()
            f()
        t_hip, t_ref = [], []
        for _ in range(a.reps):
            ms, out_hip = timed(hip, a.iters)
            t_hip.append(ms)
            ms, out_ref = timed(ref, a.iters)
            t_ref.append(ms)
    rel = float((out_hip.double() - out_ref.double()).norm() / out_ref.double().norm())
    res = {"workload": f"MAGI ViT-VAE encoder tile, {a.depth} blocks x 1024, 16 heads x 64, {tuple(x.shape)} -> {tuple(out_hip.shape)}, bf16, "
                       "synthetic weights",
           "hip_ms_per_tile": spread(t_hip), "torch_ms_per_tile": spread(t_ref),
           "hip_over_torch": round(statistics.median(t_hip) / statistics.median(t_ref), 3),
           "hip_vs_torch_rel_l2": round(rel, 5), "finite": bool(torch.isfinite(out_hip.float()).all())}
    res["kernels"] = kernel_shares(ops, hip, ("gemm", "layernorm", "vit_head_prep", "vit_attention", "vit_patch_rows", "vit_latent_head"))
    print(json.dumps(res))


def blend_in_place(frames, plan):
    """The reference's chain as eager torch: every tile against its already blended neighbours, in place."""
    at, ah, aw = plan.axes
    for f, i, j in plan.tiles:
        tile = frames[f, i, j]
        if f > 0:
            blend_rows(frames[f - 1, i, j], tile, 2, at.blend)
        if i > 0:
            blend_rows(frames[f, i - 1, j], tile, 3, ah.blend)
        if j > 0:
            blend_rows(frames[f, i, j - 1], tile, 4, aw.blend)
    out = []
    for f in range(at.count):
        rows = [torch.cat([frames[f, i, j][:, :, :at.limit, :ah.limit, :aw.limit] for j in range(aw.count)], dim=4) for i in range(ah.count)]
        out.append(torch.cat(rows, dim=3))
    return torch.cat(out, dim=2)


def bench_encode_clip(a):
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.vae import HipMagiVAEDecoder, encode_prefix_video
    cfg = published_encoder_config(a)
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda")
    vae.load_synthetic(seed=0)
    fps, scale = 24, 0.5
    clip = torch.randint(0, 256, (32, 720, 1280, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3), dtype=torch.uint8)
    kw = dict(tile_sample_min_length=fps // 2, tile_sample_min_height=256, tile_sample_min_width=256, allow_spatial_tiling=True)
    plan = vae.encode_tile_plan((1, 3, 32, 720, 1280), **kw)

    def loop():
        video = clip.permute(3, 0, 1, 2).unsqueeze(0)              # uint8: the patch kernel normalises, as in (B)
        frames = {}
        for idx in plan.tiles:
            (t0, t1), (h0, h1), (w0, w1) = plan.latent_span(idx)
            frames[idx] = vae.encode(video[:, :, t0:t1, h0:h1, w0:w1], sample_posterior=False)
        return blend_in_place(frames, plan) * scale

    hip = lambda: encode_prefix_video(clip, fps, vae, scale)
    with torch.no_grad():
        for f in (loop, hip):
            f()
        t_loop, t_hip = [], []
        for _ in range(a.reps):
            ms, out_loop = timed(loop, 1)
            t_loop.append(ms)
            ms, out_hip = timed(hip, 1)
            t_hip.append(ms)
    groups = {"x".join(map(str, k)): len(v) for k, v in plan.groups().items()}
    res = {"workload": f"MAGI prefix-video encode, {a.depth} blocks x 1024, uint8 {tuple(clip.shape)} -> {tuple(out_hip.shape)}, "
                       f"{len(plan.tiles)} tiles in groups {groups}, synthetic weights",
           "tile_by_tile_ms_per_clip": spread(t_loop), "encode_prefix_video_ms_per_clip": spread(t_hip),
           "batched_over_tile_by_tile": round(statistics.median(t_hip) / statistics.median(t_loop), 3),
           "identical": bool(torch.equal(out_loop, out_hip)), "differing_values": int((out_loop != out_hip).sum()),
           "rel_l2": float((out_hip.double() - out_loop.double()).norm() / out_loop.double().norm())}
    res["kernels"] = kernel_shares(ops, hip, ("gemm", "layernorm", "vit_head_prep", "vit_attention", "vit_patch_rows", "vit_latent_head",
                                              "vit_latent_blend"))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", action="store_true", help="one config-5 chunk: tile-by-tile loop against tiled_decode_3d")
    ap.add_argument("--encode", action="store_true", help="the encoder on one 12 x 256 x 256 tile against the restated module in torch")
    ap.add_argument("--encode-clip", action="store_true", help="encode_prefix_video of a 32-frame 720 x 1280 clip against the tile loop")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--z-chans", type=int, default=16)
    a = ap.parse_args()
    if a.chunk or a.encode or a.encode_clip:
        assert torch.cuda.is_available(), "needs the GPU"
        return bench_chunk(a) if a.chunk else bench_encode_tile(a) if a.encode else bench_encode_clip(a)
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

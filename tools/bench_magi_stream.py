#!/usr/bin/env python3
"""What streaming a MAGI request costs and buys: `MagiPipeline._run` followed by a blocking copy of the returned frames to the host (what
a consumer of the unstreamed path has to do) against `run_streaming_generation(..., continuous=True)`, at BASELINE config 5's latent
(16 x 24 x 90 x 90, chunks of 6 frames, window 4, 64 steps: 112 forwards per clip) with the 720 x 720 chunk decode of
profiles/r14_magi_tiled_decode.md (24 blocks x 1024, synthetic weights, 16 tiles per chunk).

The forwards come from the stub of tools/bench_magi_pipeline.py (`--forward-ms` of device work each) or, with `--real`, from
`HipVideoDiTModel` at MAGI-4.5B's dimensions with `--real-layers` layers.  The legs alternate clip by clip in one process; the first
clip of every leg is a warm-up and is dropped; `run` and `run_again` are the A/A pair that gives the spread.  Per leg:

  clip_ms          from the start of the request until every frame is on the host
  first_frame_ms   from the start of the request until the first frame is on the host (unstreamed: the end of the blocking copy)
  push_host_ms     host time inside `MagiFrameStream.push` (unstreamed: inside `post_chunk_process`), per chunk
  decode_gap_ms    device time on the denoising stream between the hand-out (behind its integrate launch) and the point where the next
                   forward may start, per chunk: the chunk decode where it runs on that stream, nothing where it runs on its own

profiles/r23_magi_streaming.md holds the figures, among them those of the form that decoded on the denoising stream, which was measured
with this tool before it was deleted.

    python tools/bench_magi_stream.py [--clips 3] [--forward-ms 20] [--steps 64] [--depth 24]
    python tools/bench_magi_stream.py --real [--real-layers 8] [--clips 3]
    python tools/bench_magi_stream.py --pixel-format yuv420p [--clips 3]

`--pixel-format yuv420p` / `nv12` adds the legs `stream_<format>` (the blend's rgb24 frames converted on the decode stream,
`ifx_rgb8_yuv420`) and `stream_again` (the `rgb24` stream once more: the A/A pair the YUV leg is read against), with the bytes copied
per chunk.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

C, CW, H, W, CHUNKS, WINDOW = 16, 6, 90, 90, 4, 4
CAP_L, CAP_C = 800, 4096


class Embedder:
    model_max_length = CAP_L

    def __init__(self, device, length):
        self.device, self.length = device, length

    def get_text_embeddings(self, prompts):
        g = torch.Generator().manual_seed(3)
        m = torch.zeros(1, self.model_max_length)
        m[:, :100] = 1
        return torch.randn(1, self.model_max_length, self.length, generator=g).to(self.device), m.to(self.device)


def make_vae(depth: int, device):
    import magi_vit_util as U
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    cfg = U.VitConfig(video_size=256, video_length=16, patch_size=8, patch_length=4, z_chans=C, embed_dim=1024, depth=depth, num_heads=16,
                      qkv_bias=True, ln_in_attn=True, use_final_proj=True)
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device=device)
    vae.decoder.load_synthetic(seed=0)
    return vae


def make_dit(args, device):
    from bench_magi_pipeline import make_stub, real_model
    if args.real:
        dit = real_model(args.real_layers, device)
        cap_c = dit.model_config.caption_channels
    else:
        dit = make_stub(1, args.forward_ms)
        dit.model_config.in_channels, dit.model_config.caption_max_length = C, CAP_L
        cap_c = 16
        dit.w = {"y_embedder.null_caption_embedding": torch.zeros(CAP_L, cap_c, device=device)}
    rc = dit.runtime_config
    rc.num_steps, rc.window_size, rc.chunk_width, rc.temporal_downsample_factor = args.steps, WINDOW, CW, 4
    rc.num_frames, rc.video_size_h, rc.video_size_w, rc.fps, rc.scale_factor = 4 * CW * CHUNKS, 8 * H, 8 * W, 24, 1.0
    return dit, cap_c


class Probe:
    """Host and device time around every chunk's decode, whichever way it is made."""

    def __init__(self):
        self.host, self.events = [], []

    def wrap(self, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            self.host.append((time.perf_counter() - t0) * 1e3)
            e1.record()
            self.events.append((e0, e1))
            return out
        return timed

    def take(self):
        host, gaps = self.host, [a.elapsed_time(b) for a, b in self.events]
        self.host, self.events = [], []
        return host, gaps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=3, help="clips per leg (one more is run first and dropped)")
    ap.add_argument("--forward-ms", type=float, default=20.0, help="device work standing in for a model forward")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--depth", type=int, default=24, help="blocks of the ViT-VAE decoder")
    ap.add_argument("--real", action="store_true", help="forwards of HipVideoDiTModel (MAGI-4.5B's dimensions, synthetic weights)")
    ap.add_argument("--real-layers", type=int, default=8)
    ap.add_argument("--pixel-format", default="rgb24", choices=["rgb24", "yuv420p", "nv12"])
    args = ap.parse_args()
    import inferix_amd.pipeline.magi as PM
    from inferix_amd.streaming import MagiFrameStream
    dev = torch.device("cuda", torch.cuda.current_device())
    dit, cap_c = make_dit(args, dev)
    vae = make_vae(args.depth, dev)
    config = SimpleNamespace(model_config=dit.model_config, engine_config=dit.engine_config, runtime_config=dit.runtime_config)
    pipe = PM.MagiPipeline(config, dit=dit, vae=vae, embedder=Embedder(dev, cap_c))
    probe = Probe()
    PM.post_chunk_process = probe.wrap(PM.post_chunk_process)          # the unstreamed legs' decode
    first = []

    def callback(frames):
        if not first:
            first.append(time.perf_counter())
    streams = {"stream": MagiFrameStream(vae, config, slots=CHUNKS, callback=callback)}
    fmt = args.pixel_format
    if fmt != "rgb24":
        streams[f"stream_{fmt}"] = MagiFrameStream(vae, config, slots=CHUNKS, callback=callback, pixel_format=fmt)
        streams["stream_again"] = MagiFrameStream(vae, config, slots=CHUNKS, callback=callback)
    for fs in streams.values():
        fs.push = probe.wrap(fs.push)
    legs = ["run"] + list(streams) + ["run_again"]
    res = {k: {"clip": [], "first": [], "host": [], "gap": []} for k in legs}
    frames_out = {}
    for clip in range(args.clips + 1):
        for leg in legs:
            first.clear()
            torch.manual_seed(clip)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if leg in streams:
                pipe.run_streaming_generation(["a prompt"], callback, num_segments=1, continuous=True, frame_stream=streams[leg],
                                              keep_video=False)
                t1 = time.perf_counter()
                t_first = first[0]
                frames_out[leg] = streams[leg]._slots[-1].views[0].clone()                          # the last chunk's frames
                if streams[leg].pixel_format == "rgb24":
                    frames_out[leg] = frames_out[leg].permute(0, 3, 1, 2)
            else:
                host = pipe._run("a prompt", None, "unused").cpu()
                t1 = t_first = time.perf_counter()
                frames_out[leg] = host[-host.shape[0] // CHUNKS:]
            torch.cuda.synchronize()
            host_ms, gaps = probe.take()
            assert len(host_ms) == CHUNKS, (leg, len(host_ms))
            if clip == 0:
                continue
            r = res[leg]
            r["clip"].append((t1 - t0) * 1e3)
            r["first"].append((t_first - t0) * 1e3)
            r["host"].extend(host_ms)
            r["gap"].extend(gaps)
    out = {"forwards": f"HipVideoDiTModel x {args.real_layers} layers" if args.real else f"stub, {args.forward_ms} ms",
           "steps_per_clip": args.steps + (CHUNKS - 1) * args.steps // WINDOW, "clips": args.clips, "vae_depth": args.depth,
           "device": torch.cuda.get_device_name(dev),
           "frames_equal": {k: bool(torch.equal(frames_out[k], frames_out["run"])) for k in legs[1:] if k != f"stream_{fmt}"}}
    if fmt != "rgb24":                                   # the YUV leg against the same conversion of the unstreamed frames
        from inferix_amd import hip_ops
        from inferix_amd.streaming import PIXEL_FORMATS
        want = hip_ops.rgb8_to_yuv420(frames_out["run"].permute(0, 2, 3, 1).contiguous().to(dev), layout=PIXEL_FORMATS[fmt]).cpu()
        out["frames_equal"][f"stream_{fmt}"] = bool(torch.equal(frames_out[f"stream_{fmt}"], want))
        out["pixel_format"] = fmt
        out["d2h_bytes_per_chunk"] = {k: fs._slots[0].dev.numel() for k, fs in streams.items()}
    med = statistics.median
    for leg, r in res.items():
        out[leg] = {"clip_ms": [round(v, 1) for v in r["clip"]], "clip_ms_median": round(med(r["clip"]), 1),
                    "first_frame_ms_median": round(med(r["first"]), 1), "push_host_ms_median": round(med(r["host"]), 3),
                    "decode_gap_ms_median": round(med(r["gap"]), 3)}
    spread = abs(out["run"]["clip_ms_median"] - out["run_again"]["clip_ms_median"])
    out["aa_spread_ms"] = round(spread, 1)
    if fmt != "rgb24":
        out["aa_spread_stream_ms"] = round(abs(out["stream"]["clip_ms_median"] - out["stream_again"]["clip_ms_median"]), 1)
    out["first_frame_ratio"] = round(out["stream"]["first_frame_ms_median"] / out["run"]["first_frame_ms_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

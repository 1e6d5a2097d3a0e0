"""Per-block streaming, measured: the per-block callback as upstream has it (`continuous=False`: every block decoded as a clip of its
own, fp32 finishing chain, synchronous `.cpu()`) against `continuous=True` (inferix_amd/streaming.py: one decoder stream, uint8 finished
on the device, asynchronous copy), alternating in ONE process on the full-size synthetic model and VAE (Wan 1.3B, 480p, one 21-latent
segment = 7 blocks of 3), after a warm-up.  `continuous` keeps nothing on the host (`keep_video=False`); `continuous_keep` keeps an
unpinned copy of every block and builds the segment's video inside the timed region, as the parent's segment does with its fp32 frames.
A last mode, `none`, runs the same segment with a block callback that only records the events: the denoising loop with nothing between
its blocks, which is what the gaps of the others are read against.

    python tools/bench_stream.py [--rounds 3] [--layers 30] [--out stream.json]
    python tools/bench_stream.py --pixel-format yuv420p [--rounds 5]

`--pixel-format yuv420p` / `nv12` measures the YUV 4:2:0 streams instead: the legs are `continuous` (`rgb24`, the yardstick),
`continuous_<format>`, `continuous_again` (`rgb24` once more: the A/A pair that gives the spread) and `none`, and a `kernels` section times
`ifx_frames_yuv420` against `ifx_frames_u8` on one 12-frame 480 x 832 block, launch by launch between a pair of events, alternating
`u8`, the format's layout, `u8_again` over inputs that rotate through more bytes than the Infinity Cache holds (medians, bytes from the
shapes, share of the 8.0 TB/s HBM peak).

Per block b (events on the denoising stream unless said otherwise):
    x0[b]      recorded on entry to the block callback: the block's last denoise step is in the queue in front of it
    end[b]     recorded on return from the block callback: the block's decode (if any) is in front of it
  host_ms      host clock around the callback.  `parent` synchronises inside it (`frames.cpu()` is a blocking copy: the host waits for the
               block's denoise + decode + copy); `continuous` does not, unless all slots are in flight
  denoise_ms   elapsed(end[b], x0[b+1]): the next block's denoise steps as the device saw them, INCLUDING any time the device stood
               idle because the host had not enqueued them yet
  gap_ms       denoise_ms - median denoise_ms of `none` for the same block index: the device gap between the last kernel of a block
               and the first denoise kernel of the next (a difference of two event intervals; negative values are noise)
  ready_ms     x0[b] -> the block's frames readable on the host: `parent` elapsed(x0[b], end[b]) (`.cpu()` has returned when end[b] is
               recorded), `continuous` elapsed(x0[b], copied[b]) with `copied` the FrameStream's event on its copy stream
Per segment: wall time (host clock, device synchronised at both ends, frames flushed), per block and per emitted video frame (`parent`
emits 9 frames per block, `continuous` 9 + 12 + 12 + ...), and the D2H bytes per block from the shapes."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAN_1_3B = dict(patch_size=[1, 2, 2], text_len=512, in_dim=16, dim=1536, ffn_dim=8960, freq_dim=256, text_dim=4096, out_dim=16,
                num_heads=12, num_layers=30, eps=1e-6)
LATENT = [16, 60, 104]
SEGMENT, BLOCK = 21, 3


def build(layers):
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.vae import HipWanVAEWrapper, synthetic_decoder_state_dict
    from inferix_amd.wan import HipCausalWanModel, HipWanDiffusionWrapper
    from inferix_amd.wan.synthetic import synthetic_state_dict
    mk = dict(WAN_1_3B, num_layers=layers)
    model = HipCausalWanModel(**{**mk, "patch_size": tuple(mk["patch_size"])}, device="cuda:0")
    model.load_state_dict(synthetic_state_dict(model, seed=0))
    gen = HipWanDiffusionWrapper(model=model, timestep_shift=5.0)
    pe = torch.zeros(1, 512, 4096)
    pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(1))
    pe = pe.to(torch.bfloat16).cuda()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=BLOCK,
                independent_first_frame=False, context_noise=0, frame_seq_length=1560, kv_cache_tokens=32760, latent_shape=LATENT)
    vae = HipWanVAEWrapper(synthetic_decoder_state_dict(seed=0))
    return SelfForcingPipeline(conf, text_encoder=lambda text_prompts: {"prompt_embeds": pe.expand(len(text_prompts), -1, -1)},
                               vae=vae, generator=gen)


class Probe:
    """Wraps the block callback of the inner pipeline's `inference` for one segment."""

    def __init__(self):
        self.x0, self.end, self.host_ms = [], [], []

    def wrap(self, cb):
        def block_callback(block_latent, block_index):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            if cb is not None:
                cb(block_latent, block_index)
            self.host_ms.append((time.perf_counter() - t0) * 1e3)
            e1.record()
            self.x0.append(e0)
            self.end.append(e1)
        return block_callback


def run_segment(pipe, mode, streams):
    stream = streams.get(mode)
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    probe = Probe()
    inner = pipe.pipeline.inference

    def hooked(**kw):
        kw["block_callback"] = probe.wrap(kw.get("block_callback"))
        return inner(**kw)
    emitted = []
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if mode == "none":
        kvm, reqs = KVCacheManager(device=pipe.device), [KVCacheRequest("bench_req")]
        inner(noise=pipe._noise(1, SEGMENT), text_prompts=["synthetic"], return_latents=True, kv_cache_manager=kvm,
              kv_cache_requests=reqs, block_callback=probe.wrap(None), decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=True)
        for r in reqs:
            if r.request_id in kvm.request_to_kv_caches:
                kvm.free(r)
    else:
        pipe.pipeline.inference = hooked
        try:
            if stream is not None:
                stream.reset()
                stream.events.clear()
                stream.callback = lambda f: emitted.append(f.shape[0])
                pipe._generate_segment_with_streaming("synthetic", None, None, segment_length=SEGMENT, continuous=True,
                                                      frame_stream=stream)
                stream.video()                        # flushes; with keep=True also the concatenation the parent's return value has
            else:
                pipe._generate_segment_with_streaming("synthetic", None, lambda f: emitted.append(f.shape[0]), segment_length=SEGMENT)
        finally:
            del pipe.pipeline.inference
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    nb = len(probe.x0)
    print(f"{mode}: {wall:.1f} ms, {nb} blocks, {sum(emitted)} frames", file=sys.stderr, flush=True)
    rec = dict(mode=mode, wall_ms=wall, blocks=nb, frames=sum(emitted), host_ms=probe.host_ms,
               denoise_ms=[probe.end[b].elapsed_time(probe.x0[b + 1]) for b in range(nb - 1)],
               decode_ms=[probe.x0[b].elapsed_time(probe.end[b]) for b in range(nb)])
    if stream is not None:
        rec["ready_ms"] = [probe.x0[b].elapsed_time(stream.events[b][1]) for b in range(nb)]
    elif mode == "parent":
        rec["ready_ms"] = list(rec["decode_ms"])
    return rec


def kernel_level(layout, launches=100, buffers=10):
    """One 12-frame 480 x 832 block through `frames_u8` and `frames_yuv420`, every launch between two events; `buffers` x 28.8 MB of
    input in rotation, so that no launch finds its input in the 256 MB Infinity Cache."""
    from inferix_amd import hip_ops
    T, H, W = 12, 8 * LATENT[1], 8 * LATENT[2]
    xs = [torch.randn(T, H, W, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(k)).to(torch.bfloat16)
          for k in range(buffers)]
    out_u8 = torch.empty(T, H, W, 3, dtype=torch.uint8, device="cuda")
    out_yuv = torch.empty(T, H * 3 // 2, W, dtype=torch.uint8, device="cuda")
    legs = {"u8": lambda x: hip_ops.frames_u8(x, out=out_u8),
            layout: lambda x: hip_ops.frames_yuv420(x, out=out_yuv, layout=layout),
            "u8_again": lambda x: hip_ops.frames_u8(x, out=out_u8)}
    nbytes = {"u8": 9.0 * T * H * W, layout: 7.5 * T * H * W, "u8_again": 9.0 * T * H * W}
    events = {k: [] for k in legs}
    busy = torch.randn(8192, 8192, device="cuda").to(torch.bfloat16)
    torch.cuda.synchronize()
    for _ in range(40):                               # device work for the host to run ahead of: no interval below waits for a launch
        busy @ busy
    for i in range(launches + 10):                    # the first ten rounds are the warm-up
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(xs[i % buffers])
            e1.record()
            if i >= 10:
                events[k].append((e0, e1))
    torch.cuda.synchronize()
    assert torch.equal(hip_ops.rgb8_to_yuv420(out_u8, layout=layout), out_yuv)
    res = {"block": [T, H, W], "launches": launches, "hbm_peak_tb_s": 8.0}
    for k, ev in events.items():
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
        med = statistics.median(us)
        res[k] = dict(us=spread(us), bytes=int(nbytes[k]), tb_s=round(nbytes[k] / med * 1e-6, 3),
                      hbm_peak_fraction=round(nbytes[k] / med * 1e-6 / 8.0, 3))
    res["u8_spread_us"] = round(abs(res["u8"]["us"]["median"] - res["u8_again"]["us"]["median"]), 3)
    return res


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 3), min=round(xs[0], 3), max=round(xs[-1], 3), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pixel-format", default="rgb24", choices=["rgb24", "yuv420p", "nv12"],
                    help="yuv420p / nv12: the YUV legs against the rgb24 stream (an A/A pair of it for the spread) and the kernel timing")
    a = ap.parse_args()
    from inferix_amd.streaming import PIXEL_FORMATS, FrameStream
    pipe = build(a.layers)
    fmt = a.pixel_format
    # `continuous`: nothing kept on the host (keep_video=False); `continuous_keep`: an unpinned copy of every block and the concatenated
    # video at the end, inside the timed region — what the parent's segment does with its fp32 frames
    streams = {"continuous": FrameStream(pipe.pipeline.vae, num_samples=1, slots=3, timing=True),
               "continuous_keep": FrameStream(pipe.pipeline.vae, num_samples=1, slots=3, timing=True, keep=True)}
    modes = ("parent", "continuous", "continuous_keep", "none")
    if fmt != "rgb24":
        streams = {"continuous": FrameStream(pipe.pipeline.vae, num_samples=1, slots=3, timing=True),
                   f"continuous_{fmt}": FrameStream(pipe.pipeline.vae, num_samples=1, slots=3, timing=True, pixel_format=fmt),
                   "continuous_again": FrameStream(pipe.pipeline.vae, num_samples=1, slots=3, timing=True)}
        modes = tuple(streams) + ("none",)
    for m in modes:                                   # warm-up: allocations, pinned buffers, memoised plans
        run_segment(pipe, m, streams)
    runs = [run_segment(pipe, m, streams) for _ in range(a.rounds) for m in modes]
    by = {m: [r for r in runs if r["mode"] == m] for m in modes}
    nb = by["none"][0]["blocks"]
    base = [statistics.median(r["denoise_ms"][b] for r in by["none"]) for b in range(nb - 1)]
    H, W = 8 * LATENT[1], 8 * LATENT[2]
    out = dict(device=torch.cuda.get_device_name(0), layers=a.layers, rounds=a.rounds, segment_latents=SEGMENT, blocks=nb,
               d2h_bytes_per_block=dict(parent=9 * H * W * 3 * 4, continuous_first=9 * H * W * 3, continuous=12 * H * W * 3),
               denoise_ms_none_by_block=[round(x, 3) for x in base], modes={})
    if fmt != "rgb24":
        out["pixel_format"] = fmt
        out["d2h_bytes_per_block"] = dict(continuous_first=9 * H * W * 3, continuous=12 * H * W * 3,
                                          **{f"continuous_{fmt}_first": 9 * H * W * 3 // 2, f"continuous_{fmt}": 12 * H * W * 3 // 2})
        out["slot_bytes"] = {m: sum(s.dev.numel() for s in fs._slots) for m, fs in streams.items()}
        out["kernels"] = kernel_level(PIXEL_FORMATS[fmt])
    for m in modes:
        rs = by[m]
        d = dict(frames_per_segment=rs[0]["frames"], wall_ms=spread([r["wall_ms"] for r in rs]),
                 wall_ms_per_block=spread([r["wall_ms"] / nb for r in rs]),
                 host_ms_in_callback=spread([x for r in rs for x in r["host_ms"]]),
                 host_ms_in_callback_by_block=[round(statistics.median(r["host_ms"][b] for r in rs), 3) for b in range(nb)],
                 denoise_ms=spread([x for r in rs for x in r["denoise_ms"]]),
                 gap_ms=spread([r["denoise_ms"][b] - base[b] for r in rs for b in range(nb - 1)]),
                 callback_span_ms=spread([x for r in rs for x in r["decode_ms"]]))
        if rs[0]["frames"]:
            d["wall_ms_per_frame"] = spread([r["wall_ms"] / r["frames"] for r in rs])
            d["frames_per_s"] = spread([1e3 * r["frames"] / r["wall_ms"] for r in rs])
        if "ready_ms" in rs[0]:
            d["ready_ms"] = spread([x for r in rs for x in r["ready_ms"]])
            d["ready_ms_per_frame"] = spread([x / (r["frames"] / nb if m == "parent" else (9 if b == 0 else 12))
                                              for r in rs for b, x in enumerate(r["ready_ms"])])
        out["modes"][m] = d
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

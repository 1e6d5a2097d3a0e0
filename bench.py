#!/usr/bin/env python3
"""bench.py — Self-Forcing 480p block-diffusion denoising throughput on MI355X.

    python bench.py --gpus N --steps K --warmup W

One "step" = one full pass of the hot path over one batch of synthetic input: a 21-latent-frame clip
(1 x 21 x 16 x 60 x 104), block_size 3 -> 7 blocks x (4 denoise steps + 1 clean-context re-run) = 35
generator forwards of the 30-layer Wan2.1-1.3B causal DiT with a growing KV prefix (4680 ... 32760 keys) in the
KV manager's per-request cache (an `ifx_kv_view` with the identity page map; the page-table form of the same
cache is timed in the `streaming_steady` leg: within 2 % of it).  Text encoder and VAE are outside the path (prompt embeddings are synthetic,
decode_mode = NO_DECODE; the per-block callback receives latents).  Inputs/weights are resident in HBM
before the timed region.

N > 1: the clip is sharded along the per-frame spatial token axis (sequence/context parallel, RCCL K/V
all-gather per layer) -> fixed total work, "scaling": "strong".

Prints ONE JSON line on rank 0 (driver contract).  A plain run only sets up, warms up, times the K steps and prints the
headline figure; `--full` adds everything else measured beside it after the timed region: `roofline` (block-causal attention
kernel, MFMA-bound), `roofline_gemm`, the shader clock, per-block timings, the decode / text-encoder / config legs and
`cpu_baseline` (CPU oracle timed on the host cores, N=1 only) with its parity check.  `--dump-outputs DIR` writes the latents
of the last timed step to DIR/latents.npy (float32); inputs, weights and the re-noising draws are seeded, so runs with the same
arguments are comparable output for output.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: required by RCCL on this driver stack
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    # a sequence-parallel rank runs two launch chains + two exchange streams whose wait kernels spin on device: with the runtime's
    # default of 4 hardware queues torch's pool streams share queues (tools/probe_stream_queues.py: pool2 / pool3, pool0 / pool5 ...)
    # and everything enqueued behind a spinning wait in the same queue stands still; 8 queues keep the first five streams apart
    # (measured neutral on one GPU: profiles/r5_stream_queues.md)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch  # noqa: E402

# gfx950 peaks (MI355X_MICROARCH.md): dense bf16 MFMA ~2.5 PFLOP/s, HBM3E 8 TB/s
PEAK_BF16_TFLOPS = 2500.0
PEAK_HBM_GBPS = 8000.0

WAN_1_3B = dict(patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=1536, ffn_dim=8960, freq_dim=256,
                text_dim=4096, out_dim=16, num_heads=12, num_layers=30, eps=1e-6)
LATENT = (16, 60, 104)         # 480p: 480x832 pixels / 8
FRAMES, BLOCK = 21, 3
STEPS_LIST = [1000, 750, 500, 250]


def build_pipeline(device, parallel_config=None, num_layers=None):
    from inferix_amd.pipeline import CausalInferencePipeline
    from inferix_amd.wan import HipCausalWanModel, HipWanDiffusionWrapper
    from inferix_amd.wan.synthetic import synthetic_state_dict
    cfg = dict(WAN_1_3B)
    if num_layers:
        cfg["num_layers"] = num_layers
    model = HipCausalWanModel(**cfg, parallel_config=parallel_config, device=device)
    model.load_state_dict(synthetic_state_dict(model, seed=0))
    gen = HipWanDiffusionWrapper(model=model, timestep_shift=5.0, parallel_config=parallel_config)
    args = SimpleNamespace(denoising_step_list=STEPS_LIST, warp_denoising_step=True, num_frame_per_block=BLOCK,
                           independent_first_frame=False, context_noise=0, frame_seq_length=1560,
                           kv_cache_tokens=32760)
    g = torch.Generator().manual_seed(1)
    pe = torch.zeros(1, 512, 4096)
    pe[:, :40] = torch.randn(1, 40, 4096, generator=g)
    pe = pe.to(torch.bfloat16).to(device)
    pipe = CausalInferencePipeline(args, device, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe},
                                   vae=None, parallel_config=parallel_config)
    return model, gen, pipe


def cpu_baseline(layers: int = 30, gpu_leg=None):
    """BASELINE config 1 on this box's host cores, MEASURED end to end (nothing interpolated): Self-Forcing 480p, block_size 3,
    ONE denoise step (`denoising_step_list=[1000]`) + the clean-context re-run, one block of 3 latent frames, all 30 layers,
    NO_DECODE — `O.inference` of the CPU oracle (the port of the reference's CPU / PyTorch path that tests pin to the
    reference bit for bit).  About 60-90 s of CPU work.  value = 3 latent frames / wall time of the two generator forwards."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import wan_oracle as O
    cfg = O.WanConfig(num_layers=layers)
    # `gpu_leg(W)` (config1_gpu: the HIP path on the SAME seeded weights, noise and prompt) returns the HIP latents of this config: the
    # oracle is then also the CHECKER of the full-size, full-depth result of this very run — `parity_vs_gpu` below — not only the thing
    # timed.  The weights are the ones the reference-generated fixture tests/golden/config1_full.npz was made with.
    W = O.init_weights(cfg, seed=0)
    gpu = gpu_leg(W) if gpu_leg is not None and layers == 30 else None
    gpu_out = gpu.pop("_out", None) if gpu is not None else None
    weights = W if gpu_out is not None else None
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(1, BLOCK, *LATENT, generator=g).to(torch.bfloat16)
    pe = torch.zeros(1, cfg.text_len, cfg.text_dim)
    pe[:, :40] = torch.randn(1, 40, cfg.text_dim, generator=torch.Generator().manual_seed(1))
    pe = pe.to(torch.bfloat16)
    # (round-4 verdict: 0.041-0.053 frames/s between boxes and runs.)  One untimed single-layer pass pages in the math libraries and
    # the thread pool; then up to two timed runs — the second only while the leg stays inside ~100 s — and the MINIMUM is reported,
    # both wall times beside it.
    if layers > 1:
        cfg1 = O.WanConfig(num_layers=1)
        with torch.no_grad():
            O.inference(O.init_weights(cfg1, seed=0), cfg1, noise, list(pe), [1000], shift=5.0, num_frame_per_block=BLOCK)
    runs = []
    for _ in range(2):
        t0 = time.perf_counter()
        with torch.no_grad():
            out, _ = O.inference(W, cfg, noise, list(pe), [1000], shift=5.0, num_frame_per_block=BLOCK)
        runs.append(time.perf_counter() - t0)
        assert torch.isfinite(out.float()).all()
        if runs[0] > 50.0:
            break
    dt = min(runs)
    extra = {} if layers == 30 else {"INVALID": f"debug run with {layers} of 30 layers"}
    if gpu_out is not None and weights is not None:
        # HARD CHECK (round-5 verdict, item 3): the HIP path's config-1 latents of THIS run against (a) this CPU oracle run and (b) the
        # fixture the REFERENCE's own pipeline produced on the same seeded weights, noise and prompt (tests/golden/config1_full.npz,
        # oracle/gen_golden_config1_full.py), both held to 1.25 x floor + 5e-4 with the floor the fixture measured (reference vs the same
        # rollout with exact attention).  A failure marks the line and makes bench.py exit non-zero.
        from fixture_io import golden
        a, b = gpu_out.detach().cpu().double(), out.double()
        rel = float((a - b).norm() / b.norm())
        par = {"rel_l2": round(rel, 6), "max_abs": round(float((a - b).abs().max()), 5), "rms_ref": round(float(b.pow(2).mean().sqrt()), 5)}
        try:
            fx = golden("config1_full.npz")
            floor = float(fx["floor"])
            bound = 1.25 * floor + 5e-4
            ref, exact = fx["out"].double(), fx["out_exact"].double()
            same_inputs = int(noise.view(torch.int16).to(torch.int64).sum()) == int(fx["noise_checksum"]) and \
                int(pe.view(torch.int16).to(torch.int64).sum()) == int(fx["prompt_checksum"])
            par.update({"floor": round(floor, 6), "bound": round(bound, 6), "fixture_inputs_match": bool(same_inputs),
                        "oracle_here_vs_reference_fixture_rel_l2": round(float((b - ref).norm() / ref.norm()), 8),      # 0 on the generating host; other core counts move the CPU's fp32 summation order
                        "rel_l2_vs_reference_fixture": round(float((a - ref).norm() / ref.norm()), 6),
                        "rel_l2_vs_exact_attention": round(float((a - exact).norm() / exact.norm()), 6)})
            par["ok"] = bool(same_inputs and rel <= bound and par["rel_l2_vs_reference_fixture"] <= bound and par["rel_l2_vs_exact_attention"] <= bound)
        except Exception as e:                         # (a missing fixture must not hide the line; it fails the check)
            par.update({"ok": False, "error": f"{type(e).__name__}: {e}"})
        par["what"] = ("latents of config 1 (1 denoise step + context re-run, 4680 tokens, 30 layers): HIP path vs this CPU oracle run and vs the "
                       "reference-generated fixture tests/golden/config1_full.npz (same seeded weights, noise, prompt); ASSERTED: every distance "
                       "<= 1.25 x floor + 5e-4, floor = the reference's own distance from the exact-attention rollout")
        extra["parity_vs_gpu"] = par
    if gpu is not None:
        extra["gpu_same_config"] = gpu
        extra["gpu_same_config_frames_per_s"] = gpu["latent_frames_per_s"]
    return {**extra, "value": BLOCK / dt, "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": "BASELINE config 1, measured: Self-Forcing 480p, block_size 3, 1 denoise step + clean-context re-run = 2 "
                      "generator forwards of the 30-layer Wan2.1-1.3B causal DiT over one 3-frame block (N = L_kv = 4680), "
                      f"NO_DECODE, bf16 CPU oracle (O.inference); {dt:.1f} s wall",
            "seconds": round(dt, 2), "runs_s": [round(r, 2) for r in runs], "ms_per_generator_forward": round(dt / 2 * 1e3, 1), "host_cpus": os.cpu_count()}


class ClockSampler:
    """Shader clock and socket power of GPU `index` while the timed region runs: a side thread polls `rocm-smi --json` (sysfs reads, no GPU
    work) every 0.2 s.  Reported beside the roofline because every MFMA-heavy launch of this path sits at the socket power limit and the
    clock is what gives (profiles/r2_clocks_power.md): `peak` is quoted at 2.4 GHz, `frac_at_clock` scales it to the clock that was sustained.
    Never fatal: any failure yields nulls."""

    def __init__(self, index: int = 0):
        import threading
        self.index, self.samples, self._stop = index, [], threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        import re
        import subprocess
        smi = "/opt/rocm/bin/rocm-smi"
        while not self._stop.is_set():
            try:
                r = subprocess.run([smi, "-d", str(self.index), "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=3)
                card = next(iter(json.loads(r.stdout).values()))
                clk = next((v for k, v in card.items() if k.startswith("sclk")), None)
                pw = next((v for k, v in card.items() if "ower" in k and "(W)" in k), None)
                m = re.search(r"([0-9.]+)", str(clk))
                self.samples.append((float(m.group(1)) if m else None, float(pw) if pw is not None else None))
            except Exception:  # noqa: BLE001
                pass
            self._stop.wait(0.2)

    def __enter__(self):
        if os.path.exists("/opt/rocm/bin/rocm-smi"):
            self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._th.is_alive():
            self._th.join(timeout=5)

    def summary(self):
        import statistics
        clk = [c for c, _ in self.samples[1:] if c]          # the first sample may predate the first launch
        pw = [p for _, p in self.samples[1:] if p]
        return {"sclk_mhz_median": statistics.median(clk) if clk else None, "socket_power_w_median": statistics.median(pw) if pw else None,
                "samples": len(clk)}


def _sources_sha(paths):
    import hashlib
    h = hashlib.sha256()
    for p in paths:
        f = os.path.join(ROOT, p)
        if not os.path.exists(f):
            return None
        h.update(open(f, "rb").read())
    return h.hexdigest()


def _pmc_section(name):
    """One section of profiles/pmc_traffic.json (written by tools/update_pmc_traffic.py from the PMC passes of tools/profile_bench.sh),
    or (None, why) when the file is absent or was measured on different kernel sources than the ones in this tree."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None, "profiles/pmc_traffic.json absent"
    with open(path) as f:
        t = json.load(f).get(name)
    if t is None:
        return None, f"profiles/pmc_traffic.json has no '{name}' section: re-run tools/profile_bench.sh"
    srcs = t.get("kernel_sources") or [t.get("kernel_source", "inferix_amd/csrc/ifx_attn_pp.hip")]
    if t.get("kernel_source_sha256") != _sources_sha(srcs):
        return None, f"profiles/pmc_traffic.json['{name}'] was measured on different sources ({', '.join(srcs)}): re-run tools/profile_bench.sh"
    return t, None


def pmc_traffic(shards):
    """HBM-side bytes per self-attention launch from the committed PMC pass (profiles/pmc_traffic.json: FETCH_SIZE /
    WRITE_SIZE of `rocprofv3 --pmc` on tools/pmc_micro.py at the clip's MEAN prefix L = 18720, N = 4680 — traffic
    is linear in L, so that launch is the clip average).  FETCH_SIZE is doubled per the gfx950 correction of
    MI355X_MICROARCH.md §HBM.  Counters cannot be collected inside this process; the figure is tied to the kernel source it was
    measured on (sha256 in the JSON) and is null when that source has changed since, when absent, or when sharded."""
    if shards != 1:
        return {"traffic": None}
    t, why = _pmc_section("attn_self")
    if t is None:
        return {"traffic": None, "traffic_note": why}
    b = (2 * t["fetch_size_kib"] + t["write_size_kib"]) * 1024.0
    return {"traffic": round(b), "traffic_unit": "B/launch", "traffic_source": t["source"], "mfma_busy": t.get("mfma_busy"),
            "traffic_kernel_source_sha256": t["kernel_source_sha256"][:16],
            "algorithmic_bytes_per_launch": 2 * (2 * 4680 * 1536 + 2 * 18720 * 1536)}


# the six GEMM launches of one block at N rows: (name, out features, in features, extra bf16 row reads of the epilogue)
BLOCK_GEMMS = (("qkv", 4608, 1536, 0), ("o+gate+res", 1536, 1536, 1), ("cross_q", 1536, 1536, 0), ("cross_o+res", 1536, 1536, 1),
               ("ffn_up+gelu", 8960, 1536, 0), ("ffn_down+gate+res", 1536, 8960, 1))


def roofline_gemm(records, rows, forwards, layers, shards):
    """The block's linear projections (46 % of a clip): HIP events around every GEMM launch of ONE extra clip behind the timed
    region, grouped by shape.  Algorithmic FLOPs 2*N*(6*d^2 + 2*d*ffn) per layer and forward; algorithmic bytes x + W + y
    (+ the residual row an epilogue reads), each once.  MFMA busy and fabric traffic come from the PMC stamp (null when stale)."""
    by = {}
    for name, s, e, fl, nb in records:
        if name == "gemm":
            d = by.setdefault((round(fl), round(nb)), [0, 0.0])
            d[0] += 1
            d[1] += s.elapsed_time(e)
    keyof = lambda g: (round(2.0 * rows * g[1] * g[2]), round(2.0 * (rows * g[2] + g[1] * g[2] + rows * g[1] * (1 + g[3]))))
    per, tot_us, tot_fl, tot_by = {}, 0.0, 0.0, 0.0
    for g in BLOCK_GEMMS:
        nm, n_out, n_in, res = g
        fl, key = 2.0 * rows * n_out * n_in, keyof(g)
        if key not in by:
            return None
        cnt, ms = by[key]
        same = sum(1 for h in BLOCK_GEMMS if keyof(h) == key)    # O + gate and cross-o + residual: same FLOPs and bytes, one bucket
        us = ms * 1e3 / cnt
        per[nm] = {"us": round(us, 2), "tflops": round(fl / us / 1e6, 1), "frac": round(fl / us / 1e6 / PEAK_BF16_TFLOPS, 4),
                   "launches": cnt // same}
        tot_us += us
        tot_fl += fl
        tot_by += key[1]
    tf = tot_fl / tot_us / 1e6
    out = {"kernel": "ifx::gemm_pp_kernel (persistent ping-pong tile; the six linear projections of a block, epilogues fused)",
           "bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4),
           "us_per_layer": round(tot_us, 1), "ms_per_clip": round(tot_us * forwards * layers / 1e3, 1), "per_launch": per,
           "algorithmic_flops_per_layer": tot_fl, "algorithmic_bytes_per_layer": tot_by,
           "note": "O + gate and cross-o + residual have the same FLOPs and bytes and are timed as one bucket: both rows carry its mean",
           "measured_on": "HIP events around every GEMM launch of ONE clip behind the timed region (kept out of `value`)"}
    t, why = _pmc_section("gemm_block") if shards == 1 else (None, "sharded run")
    if t is None:
        out.update({"traffic": None, "mfma_busy": None, "traffic_note": why})
    else:
        b = (2 * t["fetch_size_kib"] + t["write_size_kib"]) * 1024.0
        out.update({"traffic": round(b), "traffic_unit": "B/layer (FETCH_SIZE doubled per the gfx950 correction + WRITE_SIZE)",
                    "traffic_over_algorithmic": round(b / tot_by, 2), "mfma_busy": t["mfma_busy"], "traffic_source": t["source"],
                    "traffic_kernel_source_sha256": t["kernel_source_sha256"][:16]})
    return out


def vae_decode_leg():
    """The other half of the per-block latency, measured AFTER the timed region and not part of `value`:
    the Wan2.1 VAE decoder (dim 96, synthetic weights) on this GPU, (a) as the streaming pipeline calls it — one block of 3
    latent frames from a clean cache -> 9 video frames — and (b) a whole 21-frame clip -> 81 frames."""
    import time
    from inferix_amd import hip_ops as ops
    from inferix_amd.vae import HipWanVAEWrapper, synthetic_decoder_state_dict
    vae = HipWanVAEWrapper(synthetic_decoder_state_dict(seed=0))
    lat = torch.randn(1, FRAMES, *LATENT, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, out

    blk_ms, blk = timed(lambda: vae.decode_to_pixel(lat[:, :BLOCK], use_cache=True, chunk_size=1), 3)
    clip_ms, vid = timed(lambda: vae.decode_to_pixel(lat, use_cache=True, chunk_size=BLOCK), 2)
    t = ops.KernelTimer(names=("conv3d",))
    ops.set_kernel_timer(t)
    vae.decode_to_pixel(lat, use_cache=True, chunk_size=BLOCK)
    ops.set_kernel_timer(None)
    cs = t.summary()["conv3d"]
    # shader clock while the decoder runs (the conv kernels sit at the socket power limit like the attention kernel: the fraction of the
    # peak AT THE SUSTAINED CLOCK is reported beside the contract figure against the nominal 2.4 GHz peak)
    with ClockSampler(0) as clocks:
        for _ in range(4):
            vae.decode_to_pixel(lat, use_cache=True, chunk_size=BLOCK)
        torch.cuda.synchronize()
    ck = clocks.summary()
    conv_tf = cs["flops"] / (cs["ms"] * 1e-3) / 1e12
    at_clock = round(conv_tf / (PEAK_BF16_TFLOPS * ck["sclk_mhz_median"] / 2400.0), 4) if ck.get("sclk_mhz_median") else None
    return {"clocks": ck, "conv_frac_at_clock": at_clock,
            "workload": f"Wan2.1 VAE decoder (dim 96), latent {LATENT[1]}x{LATENT[2]} -> {vid.shape[-2]}x{vid.shape[-1]} px, bf16, "
                        "synthetic weights; includes the fp32 [-1,1] pixel hand-off",
            "ms_per_block_streaming": round(blk_ms, 2), "video_frames_per_block": int(blk.shape[1]),
            "ms_per_clip": round(clip_ms, 1), "video_frames_per_clip": int(vid.shape[1]),
            "video_frames_per_s": round(vid.shape[1] / clip_ms * 1e3, 1),
            "conv_launches": cs["launches"], "conv_tflops": round(cs["flops"] / (cs["ms"] * 1e-3) / 1e12, 1),
            "conv_frac_of_bf16_peak": round(cs["flops"] / (cs["ms"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}


def per_block_decode_leg(clip_with_callback):
    """BASELINE config 2 end to end (PER_BLOCK): the same clip with every finished block handed to the VAE decoder the way the
    streaming pipeline does (`decode_to_pixel(block, use_cache=True, chunk_size=1)` from the block callback).  Measured AFTER the
    timed region; `value` keeps SURVEY §8d's definition (generator calls only)."""
    import time
    from inferix_amd.vae import HipWanVAEWrapper, synthetic_decoder_state_dict
    vae = HipWanVAEWrapper(synthetic_decoder_state_dict(seed=0))
    frames = []

    side = torch.cuda.Stream() if os.environ.get("IFX_BENCH_DECODE_STREAM") == "1" else None   # lab A/B (see the note below)

    def cb(block_latent, block_index):
        if side is None:
            frames.append(vae.decode_to_pixel(block_latent, use_cache=True, chunk_size=1))
            return
        side.wait_stream(torch.cuda.current_stream())
        block_latent.record_stream(side)
        with torch.cuda.stream(side):
            frames.append(vae.decode_to_pixel(block_latent, use_cache=True, chunk_size=1))

    # (decoding block b on a second HIP stream while block b + 1 is denoised — IFX_BENCH_DECODE_STREAM=1 — was measured in round 1
    #  (1494.8 vs 1498.9 ms per clip) and again in round 5 (1284.0-1284.4 vs 1280.1-1281.6, tools/scratch/r5_ab_decode_stream.sh):
    #  both workloads fill the chip at the power limit, the streams serialise)
    clip_with_callback(cb)
    torch.cuda.synchronize()
    frames.clear()
    t0 = time.perf_counter()
    clip_with_callback(cb)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    n_video = sum(int(f.shape[1]) for f in frames)
    del vae
    torch.cuda.empty_cache()
    return {"workload": "config 2 end to end: 7 blocks x (4 denoise + 1 context forwards + per-block VAE decode to 480x832 pixels)",
            "ms_per_clip": round(ms, 1), "latent_frames_per_s": round(FRAMES / ms * 1e3, 3), "video_frames": n_video,
            "video_frames_per_s": round(n_video / ms * 1e3, 1)}


def streaming_steady_leg(model, gen, device, blocks: int = 20):
    """The path's product use (base_pipeline.py:468-615; the reference's only published figure is the illustrative "~500 ms per block" of
    example/streaming/README.md:124): a LONG stream with local attention — `local_attn_size = 21` frames (a 32760-token cache), `sink_size =
    3` — so that from the eighth block on the cache is saturated and EVERY block evicts one block's worth of rows behind the sink
    (causal_model.py:278-300), every finished block decoded to pixels from the block callback (PER_BLOCK).  `blocks` blocks of 3 latent
    frames; the steady state = blocks 8 .. end.  Run twice per eviction form: page-table rotation (one-frame pages: nothing moves) and
    the shift kernel (`ifx_kv_roll`, contiguous cache).  Measured AFTER the timed region on the same model object (its two attributes
    are put back).  ms per block = 4 denoise forwards + the clean-context re-run (+ decode); per-block times from events recorded in the
    block callback."""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    from inferix_amd.vae import HipWanVAEWrapper, synthetic_decoder_state_dict
    old = (model.local_attn_size, model.sink_size)
    model.local_attn_size, model.sink_size = 21, 3
    out = {"workload": f"streaming steady state: Self-Forcing 480p, local_attn_size 21 frames (32760-token cache), sink 3 frames, {blocks} blocks "
                       "x 3 latent frames, 4 denoise steps + context re-run per block, every block decoded to 12 video frames (PER_BLOCK); "
                       "steady = blocks 8.. (cache saturated, one block evicted per block)"}
    try:
        args = SimpleNamespace(denoising_step_list=STEPS_LIST, warp_denoising_step=True, num_frame_per_block=BLOCK,
                               independent_first_frame=False, context_noise=0, frame_seq_length=1560, kv_cache_tokens=None)
        pe = torch.zeros(1, 512, 4096)
        pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(1))
        pe = pe.to(torch.bfloat16).to(device)
        noise = torch.randn(1, blocks * BLOCK, *LATENT, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(device)
        vae = HipWanVAEWrapper(synthetic_decoder_state_dict(seed=0))
        for form in ("page_table_rotation", "shift_kernel"):
            pipe = CausalInferencePipeline(args, device, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
            assert pipe.local_attn_size == 21
            kvm, reqs = KVCacheManager(device), [KVCacheRequest("stream")]
            pipe._initialize_kv_cache(kvm, reqs, torch.bfloat16)
            if form == "page_table_rotation":
                for l in range(model.num_layers):
                    kvm.enable_paging(reqs[0], f"layer_{l}", 1560)
            res = {}
            for decode in (False, True):
                vae.model.clear_cache()
                marks, nvid = [], [0]

                def cb(block_latent, block_index):
                    if decode:
                        nvid[0] += int(vae.decode_to_pixel(block_latent, use_cache=True, chunk_size=1).shape[1])
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append(e)
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
                lat = pipe.inference(noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                                     decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False, block_callback=cb)
                torch.cuda.synchronize()
                assert torch.isfinite(lat.float()).all()
                ms = [a_.elapsed_time(b_) for a_, b_ in zip([e0] + marks[:-1], marks)]
                steady = ms[8:]
                key = "with_decode" if decode else "denoise_only"
                res[key] = {"ms_per_block_steady": round(sum(steady) / len(steady), 2), "ms_per_block_first7": round(sum(ms[:7]) / 7, 2),
                            "ms_per_block_max": round(max(steady), 2)}
                if decode:
                    res[key]["video_frames_per_s_steady"] = round(12.0 / (sum(steady) / len(steady)) * 1e3, 1)
                    res[key]["video_frames"] = nvid[0]
            res["ms_decode_per_block"] = round(res["with_decode"]["ms_per_block_steady"] - res["denoise_only"]["ms_per_block_steady"], 2)
            res["ms_per_generator_forward_steady"] = round(res["denoise_only"]["ms_per_block_steady"] / 5, 2)
            out[form] = res
            kvm.free(reqs[0])
            del pipe, kvm
            torch.cuda.empty_cache()
        del vae
    finally:
        model.local_attn_size, model.sink_size = old
        torch.cuda.empty_cache()
    return out


def batch_leg(model, gen, device, batch: int = 2):
    """Throughput with `batch` independent requests in ONE clip call (noise `[B, 21, 16, 60, 104]`, B prompts, B requests of the KV manager —
    the reference's batch dimension, CausalInferencePipeline.py:108-150): the row kernels and GEMMs run on B x 4680 rows, the self-attention
    once per request.  Measured AFTER the timed region; `value` stays the B = 1 clip BASELINE names.  Fills the CUs a single request's
    228-tile attention launches and 2.6-round FFN launches leave idle."""
    import time
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    args = SimpleNamespace(denoising_step_list=STEPS_LIST, warp_denoising_step=True, num_frame_per_block=BLOCK,
                           independent_first_frame=False, context_noise=0, frame_seq_length=1560, kv_cache_tokens=32760)
    g = torch.Generator().manual_seed(1)
    pe = torch.zeros(batch, 512, 4096)
    pe[:, :40] = torch.randn(batch, 40, 4096, generator=g)
    pe = pe.to(torch.bfloat16).to(device)
    pipe = CausalInferencePipeline(args, device, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
    noise = torch.randn(batch, FRAMES, *LATENT, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(device)
    kvm, reqs = KVCacheManager(device), [KVCacheRequest(f"b{i}") for i in range(batch)]
    run = lambda: pipe.inference(noise=noise, text_prompts=["synthetic"] * batch, kv_cache_manager=kvm, kv_cache_requests=reqs,
                                 decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False)
    out = run()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    t0 = time.perf_counter()
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 2 * 1e3
    for r in reqs:
        kvm.free(r)
    torch.cuda.empty_cache()
    return {"workload": f"{batch} requests in one clip call: Self-Forcing 480p, 21 latent frames each, 4 denoise steps + context re-run per block, NO_DECODE",
            "batch": batch, "ms_per_clip_call": round(ms, 1), "latent_frames_per_s_aggregate": round(batch * FRAMES / ms * 1e3, 3)}


def text_encoder_leg():
    """Time-to-first-block component of a prompt switch, measured AFTER the timed region and not part of
    `value`: umT5-XXL encoder (24 layers, dim 4096, synthetic weights generated on the device) on one 512-token prompt."""
    import time
    from inferix_amd.t5 import HipWanTextEncoder, synthetic_t5_state_dict
    enc = HipWanTextEncoder(synthetic_t5_state_dict(device="cuda"), None)
    ids = torch.randint(1, 256384, (1, 512), generator=torch.Generator().manual_seed(0))
    mask = torch.zeros(1, 512, dtype=torch.long)
    mask[:, :60] = 1
    enc.encode_ids(ids, mask)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        out = enc.encode_ids(ids, mask)["prompt_embeds"]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 5 * 1e3
    flops = 24 * (2.0 * 512 * 4096 * (4 * 4096 + 2 * 10240) + 2.0 * 512 * 10240 * 4096 + 4.0 * 64 * 512 * 512 * 64)
    del enc
    torch.cuda.empty_cache()
    return {"workload": "umT5-XXL encoder (24 layers, dim 4096, 64 heads, ffn 10240), one prompt padded to 512 tokens, bf16, "
                        "synthetic weights; tokenizer not included", "ms_per_prompt": round(ms, 2),
            "tflops": round(flops / ms / 1e9, 1), "output": list(out.shape)}


PEAK_FP8_TFLOPS = 5000.0       # dense fp8 / int8 MFMA (MI355X_MICROARCH.md)


def config1_gpu(model, gen, device, weights):
    """The GPU side of BASELINE config 1 (what `cpu_baseline` measures on the host): 1 denoise step + context re-run, one block.
    Runs on `weights` = the seeded weights the reference-generated fixture config1_full.npz was made with (`cpu_baseline` generates
    them and calls this leg) — loaded into `model` here, after every leg that times the device-generated synthetic weights."""
    from inferix_amd.core import DecodeMode
    model.load_state_dict(weights)
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    args = SimpleNamespace(denoising_step_list=[1000], warp_denoising_step=True, num_frame_per_block=BLOCK,
                           independent_first_frame=False, context_noise=0, frame_seq_length=1560, kv_cache_tokens=BLOCK * 1560)
    pe = torch.zeros(1, 512, 4096)
    pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(1))
    pe = pe.to(torch.bfloat16).to(device)
    pipe1 = CausalInferencePipeline(args, device, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
    noise = torch.randn(1, BLOCK, *LATENT, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(device)
    kvm, reqs = KVCacheManager(device), [KVCacheRequest("config1")]
    run = lambda: pipe1.inference(noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                                  decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    out = run().detach().clone()
    torch.cuda.synchronize()
    kvm.free(reqs[0])
    return {"workload": "BASELINE config 1 on the GPU: 1 denoise step + context re-run, one 3-frame block, 30 layers, NO_DECODE",
            "ms": round(ms, 2), "latent_frames_per_s": round(BLOCK / ms * 1e3, 2), "_out": out}


def quant_leg(fmt, gen, clip, rounds: int = 2, pipe_args=None):
    """BASELINE config 4: the same clip with every nn.Linear the reference's exclusion dict leaves quantised as a dynamic per-token x
    per-channel 8-bit linear (fp8 e4m3 on the fp8 MFMA / int8).  Measured AFTER the headline region on the same model object, as
    FULL un-instrumented clips interleaved with bf16 clips in the same process (bf16, 8-bit, bf16, 8-bit: the clocks of a hot part
    drift, so only adjacent clips compare — round-3 verdict; the per-launch HIP events of the breakdown used to sit inside the timed
    clip, which is where its 60 ms over GEMM + quantiser time came from).  `speedup_vs_bf16` = mean bf16 clip / mean 8-bit clip of this
    leg.  `roofline` is the 8-bit GEMM's (all launches of one separate, instrumented clip) against the dense 8-bit MFMA peak.
    Parity of the scheme: unpinned vs DAX; the wiring is pinned by the quantised-model oracle (tests/test_hip_quant.py)."""
    from inferix_amd import hip_ops as ops
    from inferix_amd import quant as Qz
    qc = (Qz.get_dynamic_fp8_per_token_act_per_channel_weight_qconfig() if fmt == "fp8"
          else Qz.get_dynamic_int8_per_token_act_per_channel_weight_qconfig())
    qdict = {"": qc, "text_embedding": None, "proj_out": None, "head": None}

    def timed_clip():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = clip()
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        return (time.perf_counter() - t0) * 1e3

    try:
        Qz.quantize_dynamic(gen, qdict)
        clip()                                            # warm: the 8-bit launches' first use
        ms_q, ms_b = [], []
        for _ in range(rounds):
            Qz.dequantize(gen)
            ms_b.append(timed_clip())
            Qz.quantize_dynamic(gen, qdict)
            ms_q.append(timed_clip())
        t = ops.KernelTimer(names=("gemm_q8", "attn_self", "quant_per_token", "layernorm"))
        ops.set_kernel_timer(t)
        pair_was = getattr(pipe_args, "pair_forwards", None)
        if pipe_args is not None:
            pipe_args.pair_forwards = False          # per-launch events: one forward at a time (see the headline's instrumented clips)
        clip()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        if pipe_args is not None:
            pipe_args.pair_forwards = pair_was
        ks = t.summary()
        gq, qa = ks["gemm_q8"], ks.get("quant_per_token", dict(ms=0.0, launches=0, bytes=0.0))
        tf = gq["flops"] / (gq["ms"] * 1e-3) / 1e12
        ms, msb = sum(ms_q) / len(ms_q), sum(ms_b) / len(ms_b)
        return {"workload": f"config 4: Self-Forcing 480p clip, {qc.name} linears + bf16 attention", "clips_run": 2 * rounds + 2,
                "ms_per_clip": round(ms, 1), "latent_frames_per_s": round(FRAMES / ms * 1e3, 3),
                "ms_per_clip_each": [round(v, 1) for v in ms_q], "bf16_ms_per_clip_interleaved": [round(v, 1) for v in ms_b],
                "speedup_vs_bf16": round(msb / ms, 4),
                "timing": "un-instrumented full clips, interleaved bf16 / 8-bit in this process; kernel sums from one more, instrumented clip",
                "roofline": {"kernel": f"ifx::gemm_pp_kernel<.., Q8> ({'e4m3' if fmt == 'fp8' else 'int8'} operands on the persistent ping-pong tile, "
                                       "per-token x per-channel dequant epilogue)", "bound": "mfma",
                             "achieved": round(tf, 1), "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_FP8_TFLOPS, 4),
                             "traffic": None, "launches": gq["launches"], "avg_launch_ms": round(gq["ms"] / gq["launches"], 4)},
                "quantiser_gbps": round(qa["bytes"] / (qa["ms"] * 1e-3) / 1e9, 1) if qa["ms"] else None,
                "quantiser_ms_per_clip": round(qa["ms"], 1), "gemm_ms_per_clip": round(gq["ms"], 1),
                "norm_quant_ms_per_clip": round(ks.get("layernorm", dict(ms=0.0))["ms"], 1),
                "attention_ms_per_clip": round(ks.get("attn_self", dict(ms=0.0))["ms"], 1),
                "parity": "bytes / scales bit-exact vs oracle/quant_oracle.py; model wiring vs the quantised-model oracle at the 1.25 x floor rule; "
                          "unpinned vs DAX (absent from the reference tree)"}
    finally:
        ops.set_kernel_timer(None)
        Qz.dequantize(gen)


def causvid_720p_leg(model, device):
    """BASELINE config 3: CausVid 720p bf16 with continuous-prompt KV rollover on the SAME 30-layer model object: latent 90 x 160
    (3600 tokens / frame, 10800 / block), `denoising_step_list=[1000, 757, 522, 0]` (last entry dropped, no warp), shift 8.0,
    3 segments of 21 latent frames, each in a NEW KVCacheRequest prefilled with the previous segment's last 3 latents
    (inferix/pipeline/causvid/pipeline.py:224-309); the pixel-space re-encode of the boundary frame is outside the timing."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.kvcache_manager import KVCacheManager
    from inferix_amd.pipeline import CausVidInferencePipeline
    from inferix_amd.wan import HipCausVidDiffusionWrapper
    H, Wd, fs = 90, 160, 3600
    gen = HipCausVidDiffusionWrapper(model=model, timestep_shift=8.0)
    args = SimpleNamespace(denoising_step_list=[1000, 757, 522, 0], warp_denoising_step=False, num_frame_per_block=BLOCK,
                           frame_seq_length=fs, kv_cache_tokens=FRAMES * fs)
    pes = []
    for i in range(3):
        pe = torch.zeros(1, 512, 4096)
        pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(10 + i))
        pes.append(pe.to(torch.bfloat16).to(device))
    table = {f"prompt {i}": pes[i] for i in range(3)}
    pipe = CausVidInferencePipeline(args, device=device, generator=gen,
                                    text_encoder=lambda text_prompts: {"prompt_embeds": table[text_prompts[0]]}, vae=None)
    g = torch.Generator().manual_seed(2)
    noises = [torch.randn(1, FRAMES, 16, H, Wd, generator=g).to(torch.bfloat16).to(device) for _ in range(3)]
    kvm = KVCacheManager(device)
    pipe.rollover(["prompt 0"], [noises[0][:, :BLOCK]], kvm, overlap_frames=BLOCK)          # warm: one block
    pipe.is_kv_cache_initialized = False
    kvm = KVCacheManager(device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = pipe.rollover(list(table), noises, kvm, overlap_frames=BLOCK)          # un-instrumented, the pipeline's default pairing
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert all(torch.isfinite(o.float()).all() for o in outs)
    # the roofline figure: ONE more segment with HIP events around every self-attention launch, forwards one at a time (a launch timed
    # while a second chain runs beside it would be charged that chain's share of the chip)
    pipe.is_kv_cache_initialized = False
    args.pair_forwards = False
    kvm = KVCacheManager(device)
    t = ops.KernelTimer(names=("attn_self",))
    ops.set_kernel_timer(t)
    pipe.rollover(["prompt 0"], [noises[0]], kvm, overlap_frames=BLOCK)
    torch.cuda.synchronize()
    ops.set_kernel_timer(None)
    args.pair_forwards = None
    ks = t.summary()["attn_self"]
    tf = ks["flops"] / (ks["ms"] * 1e-3) / 1e12
    new_frames = FRAMES + 2 * (FRAMES - BLOCK)                # segments 1, 2 regenerate nothing of their 3 prefilled frames
    fwd = 7 * 4 + 2 * (1 + 6 * 4)
    paired = bool(pipe._pairing())
    del pipe, kvm
    torch.cuda.empty_cache()
    return {"workload": "config 3: CausVid 720p (latent 90x160, block 10800 tokens, steps [1000, 757, 522], shift 8.0), 3 segments x 21 "
                        "latent frames with per-segment request rollover (3 overlap latents prefilled), 30 layers, NO decode",
            "ms_total": round(ms, 1), "ms_per_segment": round(ms / 3, 1), "generator_forwards": fwd,
            "new_latent_frames": new_frames, "latent_frames_per_s": round(new_frames / ms * 1e3, 3), "pair_forwards": paired,
            "roofline": {"kernel": "ifx::attn_fwd_pp_kernel (self-attention launches, N = 10800, L = 10800 .. 75600)", "bound": "mfma",
                         "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4),
                         "traffic": None, "launches": ks["launches"], "avg_launch_ms": round(ks["ms"] / ks["launches"], 4)}}


def magi_cp8_emulated_leg(device, cp: int = 8, layers: int = 34, fp8_quant: bool = True, steps=None, breakdown: bool = True):
    """BASELINE config 5 as a MODEL run, ONE rank of 8 emulated on one GPU (INVALID as a multi-GPU number: the all-to-alls are device
    copies of the bytes the rank would receive, inferix_amd/magi/context_parallel.py `set_cp_emulation`).  `HipVideoDiTModel` with
    MAGI-4.5B's dimensions (34 layers, hidden 3072, 24 q-heads / 8 kv-groups, ffn 12288, caption 800 x 4096; patch embedding, timestep
    and caption embedders, rope table, final norm + linear included) driven by `ChunkSchedule.run`, the reference's SampleTransport
    loop for `example/magi/configs/4.5B/4.5B_distill_quant_config.json`: 96 frames at 720 x 720 -> 4 chunks of 12150 tokens, 64
    steps in a window of 4 -> 112 denoise forwards of 1 .. 4 chunks (+ the clean chunk at the first step of stages 4 .. 6, + the
    nearly-clean re-forward), `noise2clean_kvrange = [5, 4, 3, 2]`, `cfg_number = 1`.  `fp8_quant`: layers 1 .. 32 run the
    static-scale FP8 linears.  `steps`: a subset of the schedule (debug)."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi import context_parallel as cpl
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.schedule import ChunkSchedule
    from inferix_amd.magi.types import InferenceParams
    mc = SimpleNamespace(num_layers=layers, hidden_size=3072, ffn_hidden_size=12288, num_attention_heads=24, num_query_groups=8,
                         kv_channels=128, layernorm_epsilon=1e-6, apply_layernorm_1p=True, gated_linear_unit=False,
                         cond_hidden_ratio=0.25, xattn_cond_hidden_ratio=1.0, cond_gating_ratio=1.0, patch_size=2, t_patch_size=1,
                         in_channels=16, out_channels=16, caption_channels=4096, caption_max_length=800, x_rescale_factor=1,
                         half_channel_vae=False)
    ec = SimpleNamespace(cp_size=cp, cp_strategy="cp_ulysses", fp8_quant=fp8_quant, kv_offload=False, ulysses_overlap_degree=1,
                         distill=True, shortcut_mode="8,16,16", distill_nearly_clean_chunk_threshold=0.3)
    rc = SimpleNamespace(cfg_number=1, noise2clean_kvrange=[5, 4, 3, 2], clean_chunk_kvrange=1, clean_t=0.9999, num_steps=64,
                         window_size=4, chunk_width=6)
    chunk_num, cw, lat, caption = 4, 6, 90, 100
    clip = cw * (lat // 2) ** 2
    cpl.set_cp_emulation(cp, 0)
    try:
        model = HipVideoDiTModel(SimpleNamespace(model_config=mc, engine_config=ec, runtime_config=rc), device)
        model.load_synthetic(0)
        sch = ChunkSchedule(rc.num_steps, rc.window_size, chunk_num, cw)
        g = torch.Generator(device=device).manual_seed(0)
        x0 = torch.randn(1, 16, chunk_num * cw, lat, lat, generator=g, device=device)
        x = torch.cat([x0, x0], 0)
        y = torch.randn(2, chunk_num, 800, 4096, generator=g, device=device)
        masks = torch.zeros(2, chunk_num, 800, device=device)
        masks[0, :, :caption] = 1                              # a 100-token caption; the null caption row keeps its 2 special tokens
        masks[1, :, :2] = 1
        plans = []
        sch.run(model, x.clone(), y, masks, InferenceParams(1, chunk_num * clip, device=device), steps=[0, 48, 64])   # warm: 1 chunk, 4 chunks, clean + 3 chunks
        torch.cuda.synchronize()
        # the reported time: ONE un-instrumented schedule run on a fresh InferenceParams (the per-launch HIP events of the
        # breakdown and the warm-up's cache state used to sit inside this region)
        ip = InferenceParams(1, chunk_num * clip, device=device)
        t0 = time.perf_counter()
        out = sch.run(model, x.clone(), y, masks, ip, steps=steps, on_forward=plans.append)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        # the per-kernel sums: the same run again with events around the attention / GEMM / quantiser launches
        t = ops.KernelTimer(names=("attn_magi", "gemm", "gemm_q8", "quant_static"))
        if breakdown:
            ops.set_kernel_timer(t)
            sch.run(model, x.clone(), y, masks, InferenceParams(1, chunk_num * clip, device=device), steps=steps)
            torch.cuda.synchronize()
            ops.set_kernel_timer(None)
        assert torch.isfinite(out).all()
        ks = t.summary()
        zero = {"ms": 0.0, "flops": 0.0, "launches": 0}
        at, ge = ks.get("attn_magi", zero), ks.get("gemm", zero)
        g8 = ks.get("gemm_q8", {"ms": 0.0, "flops": 0.0, "launches": 0})
        qz = ks.get("quant_static", {"ms": 0.0, "launches": 0})
        atf = at["flops"] / (at["ms"] * 1e-3) / 1e12 if at["ms"] else 0.0
        gtf = ge["flops"] / (ge["ms"] * 1e-3) / 1e12 if ge["ms"] else 0.0
        n = len(plans)
        ranges = sum(p.denoising_range_num for p in plans)
        full = steps is None
        del model
        torch.cuda.empty_cache()
        return {"workload": f"config 5 (MAGI-4.5B distill{'_quant' if fp8_quant else ''}, 96 frames 720x720 = {chunk_num} chunks x {clip} "
                            f"tokens, 64 steps, window 4), the reference's chunk schedule through the whole model, ONE rank of cp={cp} "
                            f"emulated on one GPU ({24 // cp} q-heads on 1 kv-head, 1/{cp} of the tokens through the linears); all-to-alls "
                            "replaced by device copies",
                "INVALID": "emulated rank: no xGMI transfer; not a multi-GPU measurement" + ("" if full else "; partial schedule"),
                "denoise_forwards": n, "chunk_forwards": ranges, "ms_clip_rank": round(ms, 1),
                "ms_per_denoise_forward_rank": round(ms / n, 2),
                "latent_frames_per_s_rank_view": round(chunk_num * cw / ms * 1e3, 3) if full else None,
                "chunk_tokens_per_s_rank_view": round(ranges * clip / ms * 1e3, 1),
                "attn_ms": round(at["ms"], 1), "gemm_ms": round(ge["ms"], 1),
                "roofline": {"kernel": "ifx::attn_fwd_pp_kernel (MAGI range attention, 3 q-heads on 1 kv-head)", "bound": "mfma",
                             "achieved": round(atf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(atf / PEAK_BF16_TFLOPS, 4),
                             "traffic": None, "launches": at["launches"], "avg_launch_ms": round(at["ms"] / max(at["launches"], 1), 4)},
                "timing": "ms_clip_rank: one un-instrumented schedule run on a fresh InferenceParams; attn / gemm / quantiser sums: a second, instrumented run",
                "gemm_tflops": round(gtf, 1), "fp8_quant": bool(fp8_quant),
                "gemm_fp8_ms": round(g8["ms"], 1),
                "gemm_fp8_tflops": round(g8["flops"] / (g8["ms"] * 1e-3) / 1e12, 1) if g8["ms"] else None,
                "quantiser_ms": round(qz["ms"], 1), "quantiser_launches": qz["launches"]}
    finally:
        ops.set_kernel_timer(None)
        cpl.set_cp_emulation(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer layers (makes the result INVALID)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure everything beside the headline figure (roofline clips, clocks, per-block "
                         "timings, decode / text encoder / config legs, CPU baseline and its parity check); off: the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the latents the last timed step returned to DIR/latents.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-layers", type=int, default=30, help="debug: layers of the CPU baseline run (fewer than 30 makes it INVALID)")
    ap.add_argument("--quant", choices=["none", "fp8", "int8"], default="none",
                    help="BASELINE config 4: dynamic per-token x per-channel 8-bit linears (not the headline dtype)")
    ap.add_argument("--kernel-breakdown", action="store_true", help="with --full: extra untimed clip with every kernel timed")
    ap.add_argument("--no-decode-leg", action="store_true", help="with --full: skip the VAE decode / text encoder measurements after the timed region")
    ap.add_argument("--no-config-legs", action="store_true", help="with --full: skip the config 3 / 4 / 5 legs (CausVid 720p, fp8 / int8, MAGI rank) after the timed region")
    ap.add_argument("--emulate-sp", type=int, default=0, metavar="P",
                    help="debug: time ONE rank of a P-way sequence-parallel run on one GPU, the K/V all-gather replaced "
                         "by a device copy (makes the result INVALID)")
    ap.add_argument("--sp-exchange", choices=["auto", "allgather", "peer"], default="auto",
                    help="N > 1: K/V exchange per layer — one RCCL all-gather, or direct peer stores through HIP IPC mappings; auto = peer "
                         "stores when their self-test passes on every rank, else the all-gather")
    ap.add_argument("--sp-qkv", choices=["auto", "fused", "kv-first"], default="auto",
                    help="N > 1: one fused q/k/v projection before the exchange starts, or the K/V projection first so that the exchange "
                         "runs under the q projection; auto = kv-first in front of the all-gather, fused in front of the peer stores")
    ap.add_argument("--pair", choices=["auto", "on", "off"], default="auto",
                    help="the clean-context re-run of a block enqueued layer-interleaved with the next block's first step "
                         "(pipeline pair_forwards; bit-identical results): auto = the pipeline's default (on)")
    ap.add_argument("--pair-mode", choices=["auto", "streams", "lockstep"], default="auto",
                    help="how a pair runs: two layer-interleaved launch chains on two streams, or one chain over both forwards' rows "
                         "(auto: streams)")
    ap.add_argument("--magi-leg", choices=["fp8", "bf16"], default=None,
                    help="debug: run ONLY the config 5 leg (MAGI-4.5B model through the chunk schedule, one emulated cp rank) and print it")
    ap.add_argument("--magi-steps", type=int, default=0, help="debug: with --magi-leg, only the first N steps of each schedule stage")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.kernel_breakdown and not a.full:
        ap.error("--kernel-breakdown is one of the --full measurements: add --full")
    if a.dump_outputs and a.magi_leg:
        ap.error("--dump-outputs writes the headline clip's latents; --magi-leg does not run it")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the HIP path has no CPU fallback)")
    # IFX_BENCH_SHARE_GPU=1 (test only): all ranks on cuda:0 over gloo, to exercise the N>1 code path on a 1-GPU box
    share = os.environ.get("IFX_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if a.magi_leg:
        sub = [st * 16 + i for st in range(7) for i in range(a.magi_steps)] if a.magi_steps else None
        print(json.dumps(magi_cp8_emulated_leg(device, layers=a.layers or 34, fp8_quant=a.magi_leg == "fp8", steps=sub)), flush=True)
        return
    import torch.distributed as dist
    pc = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)     # "nccl" is RCCL on ROCm
        from inferix_amd.sequence_parallel import attach_sequence_parallel
        from inferix_amd.wan import ParallelConfig
        pc = ParallelConfig(rank=rank, world_size=world, local_rank=local_rank)
    assert a.gpus == world, f"--gpus {a.gpus} but WORLD_SIZE={world} (launch with torch.distributed.run)"
    if a.emulate_sp > 1:
        assert world == 1, "--emulate-sp is a single-process debugging mode"
        from inferix_amd.wan import ParallelConfig
        pc = ParallelConfig(rank=0, world_size=a.emulate_sp, local_rank=0)

    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    model, gen, pipe = build_pipeline(device, pc, a.layers or None)
    pipe.args.pair_forwards = {"auto": None, "on": True, "off": False}[a.pair]
    model.pair_mode = None if a.pair_mode == "auto" else a.pair_mode
    exchange_used, rccl_ranks, sp_preflight = None, None, None
    if world > 1:
        from inferix_amd.sequence_parallel import PeerStoreExchange
        # a real collective first: the rank count the line reports is what an all-gather over the group saw
        seen = torch.empty(world, dtype=torch.int32, device=device)
        me = torch.tensor([rank], dtype=torch.int32, device=device)
        try:
            dist.all_gather_into_tensor(seen, me)
        except (RuntimeError, NotImplementedError):           # gloo builds without the flat form (the shared-GPU test mode)
            dist.all_gather(list(seen.view(world, 1).unbind(0)), me)
        rccl_ranks = len(set(seen.tolist()))
        peer = None
        if a.sp_exchange in ("auto", "peer"):
            try:
                peer = PeerStoreExchange(dist.group.WORLD)
                if not peer.self_test():
                    peer = None
            except Exception as exc:                 # noqa: BLE001 — IPC mapping refused on this box: fall back (all ranks agree below)
                print(f"[bench rank {rank}] peer-store exchange unavailable: {exc}", file=sys.stderr)
                peer = None
            votes = [None] * world
            dist.all_gather_object(votes, peer is not None)
            if not all(votes):
                peer = None
            if peer is None and a.sp_exchange == "peer":
                raise SystemExit("--sp-exchange peer: the peer-store self-test failed")
        attach_sequence_parallel(model, dist.group.WORLD, peer=peer, kv_first={'auto': None, 'fused': False, 'kv-first': True}[a.sp_qkv])
        # first contact with RCCL / xGMI (round-2 verdict): one layer's exchange through BOTH paths into scratch caches, compared bit
        # for bit on every rank and across ranks; a peer-store mismatch drops that path everywhere (fails closed to the all-gather),
        # an inconsistent all-gather aborts the run.  The line reports the per-exchange microseconds it measured.
        sp_preflight = model.cp.preflight(model, LATENT[1] // 2, LATENT[2] // 2, frames=BLOCK)
        if a.sp_exchange == "peer" and model.cp.peer is None and peer is not None:
            raise SystemExit(f"--sp-exchange peer: the preflight comparison failed: {sp_preflight}")
        exchange_used = "peer_store" if model.cp.peer is not None else "allgather"
        if rank == 0:
            # FIRST thing a multi-GPU run says (stderr: stdout carries the one JSON line): what the first contact with RCCL / xGMI
            # measured per exchange and which exchange the timed clips will use — a slow or fallen-back 8-GPU run is diagnosable from
            # this line alone (round-4 verdict item 9)
            print("[bench] " + json.dumps({"n_gpus": world, "rccl_ranks": rccl_ranks, "sp_exchange": exchange_used,
                                           "sp_qkv": "kv-first" if model.cp.kv_first else "fused", "sp_preflight": sp_preflight}),
                  file=sys.stderr, flush=True)
    elif a.emulate_sp > 1:
        from inferix_amd.sequence_parallel import LoopbackExchange, PeerStoreExchange, attach_sequence_parallel
        peer = PeerStoreExchange(emulate_world=a.emulate_sp) if a.sp_exchange == "peer" else None
        exchange_used = "peer_store(emulated)" if peer is not None else "allgather(emulated)"
        attach_sequence_parallel(model, exchange=LoopbackExchange(a.emulate_sp, 0), peer=peer, kv_first={'auto': None, 'fused': False, 'kv-first': True}[a.sp_qkv])
    if a.quant != "none":
        from inferix_amd import quant as Qz
        qc = (Qz.get_dynamic_fp8_per_token_act_per_channel_weight_qconfig() if a.quant == "fp8"
              else Qz.get_dynamic_int8_per_token_act_per_channel_weight_qconfig())
        Qz.quantize_dynamic(gen, {"": qc, "text_embedding": None, "proj_out": None, "head": None})
    g = torch.Generator().manual_seed(0)
    noise = torch.randn(1, FRAMES, *LATENT, generator=g).to(torch.bfloat16).to(device)
    kvm = KVCacheManager(device)
    reqs = [KVCacheRequest("bench")]
    fwd_ms = []                    # per generator forward, filled only when asked

    def clip():
        return pipe.inference(noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                              decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1 and getattr(model.cp, "peer", None) is not None:
        # one validation clip on the peer-store path before anything is timed: a wait that times out raises on every rank together
        # (PeerStoreExchange.check), and all ranks then continue on the all-gather
        try:
            clip()
            torch.cuda.synchronize()
        except RuntimeError as exc:
            print(f"[bench rank {rank}] peer-store exchange failed in the validation clip, using the all-gather: {exc}", file=sys.stderr)
            model.cp.peer, model.cp.kv_first = None, True
            exchange_used = "allgather"
            torch.cuda.synchronize()
            dist.barrier()
    # the pipeline's re-noising draws (torch.randn_like between denoise steps) come from the default generator: seeded, so that runs with
    # the same arguments see the same inputs in every step
    torch.manual_seed(0)
    for _ in range(a.warmup):
        clip()
    sync()
    with ClockSampler(local_rank if world > 1 else 0) if rank == 0 and a.full else contextlib.nullcontext() as clocks:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            out = clip()
        sync()
        dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    assert torch.isfinite(out.float()).all()
    if a.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "latents.npy"), out.float().cpu().numpy())

    forwards = a.steps * (FRAMES // BLOCK) * (len(STEPS_LIST) + 1)
    res = None
    if rank == 0:
        res = {
            "metric": "latent_frames_per_sec",
            "value": round(FRAMES * a.steps / dt, 4),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if a.quant == "none" else f"{a.quant} linears (per-token x per-channel) + bf16 attention",
            "data": "synthetic",
            "config": {"workload": "Self-Forcing 480p bf16 (Wan2.1-T2V-1.3B causal DiT, 30 layers), block_size=3, "
                                   "21 latent frames = 7 blocks x (4 denoise + 1 context) generator forwards, KV "
                                   "prefix 4680..32760 keys in the KV manager's cache (identity page map; page-table form: `streaming_steady`); `value` counts the generator calls (SURVEY 8d), the per-block VAE decode of config 2 "
                                   "is measured beside it under --full (`per_block_decode`, `vae_decode`), the text encoder in `text_encoder`",
                       "batch": 1, "latent": [FRAMES, *LATENT], "denoising_step_list": STEPS_LIST,
                       "timestep_shift": 5.0, "parallelism": f"sp{world}" if world > 1 else "single",
                       "layers": model.num_layers,
                       "pair_forwards": bool(pipe._pairing()), "pair_mode": model._pair_mode() if pipe._pairing() else None},
            "rccl_ranks": rccl_ranks, "sp_exchange": exchange_used, "sp_preflight": sp_preflight,
            "generator_forwards_timed": forwards,
        }
        if a.layers:
            res["config"]["INVALID"] = "debug run with fewer layers"
        if a.emulate_sp > 1:
            res["config"]["INVALID"] = f"one rank of sp{a.emulate_sp} emulated on one GPU, collective replaced by a copy"
    parity_failed = full_measurements(a, res, dt, clocks, model, gen, pipe, clip, noise, kvm, reqs, device, world) if a.full else False
    if rank == 0:
        print(json.dumps(res), flush=True)
    if parity_failed:
        if world > 1:
            dist.destroy_process_group()
        sys.exit(3)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def full_measurements(a, res, dt, clocks, model, gen, pipe, clip, noise, kvm, reqs, device, world):
    """--full: everything measured beside the headline figure, after the timed region, on every rank (the instrumented clips are
    collective when sharded); rank 0 adds the results to `res`.  Returns True when the config-1 parity check failed."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.core import DecodeMode
    # the timed clip's OWN per-block wall time (round-5 verdict: the instrumented figures below come from clips with the pairs off; this is
    # one more clip exactly as timed — paired forwards, no kernel timers — with one event per finished block from the block callback)
    marks = [torch.cuda.Event(enable_timing=True)]
    marks[0].record()

    def _mark(block_latent, block_index):
        e_ = torch.cuda.Event(enable_timing=True)
        e_.record()
        marks.append(e_)
    pipe.inference(noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs, decode_mode=DecodeMode.NO_DECODE,
                   free_cache_before_vae=False, block_callback=_mark)
    torch.cuda.synchronize()
    paired_block_ms = [round(x.elapsed_time(y), 2) for x, y in zip(marks[:-1], marks[1:])]

    # per-forward latency by block index (one extra untimed clip, events around each generator call)
    per_block_ms = []
    evs = []
    orig = gen.forward

    def timed_forward(**kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = orig(**kw)
        e.record()
        evs.append((kw["current_start"] // (BLOCK * 1560), s, e))
        return r
    gen.forward = timed_forward
    pair_was = getattr(pipe.args, "pair_forwards", None)
    pipe.args.pair_forwards = False      # the instrumented clips time ONE forward per interval: no layer-interleaved pairs in them
    # (round-2 verdict: the per-launch HIP events of the roofline figure are measurement overhead — they are taken on a SEPARATE clip
    #  right behind the timed region, the same launches in the same process, not inside `value`)
    timer = ops.KernelTimer(names=("attn_self",))
    breakdown = None
    if a.kernel_breakdown:
        allt = ops.KernelTimer(names=("attn_self", "attn_cross", "gemm", "gemm_q8", "quant_per_token", "layernorm",
                                      "rmsnorm_rope_append"))
        ops.set_kernel_timer(allt)
    else:
        ops.set_kernel_timer(timer)                  # the roofline clip: HIP events around every self-attention launch
    clip()
    torch.cuda.synchronize()
    ops.set_kernel_timer(None)
    if a.kernel_breakdown:
        timer = allt
        breakdown = {k: {"launches": v["launches"], "ms": round(v["ms"], 3),
                         "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] and v["flops"] else None,
                         "gbps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] else None}
                     for k, v in allt.summary().items()}
    gen.forward = orig
    # the GEMM roofline clip: events around every GEMM launch of one more clip (its own clip, so that the attention events above
    # see the launch pattern of the timed region)
    gemm_roof = None
    if a.quant == "none" and not a.layers:
        gt = allt if a.kernel_breakdown else ops.KernelTimer(names=("gemm",))
        if not a.kernel_breakdown:
            ops.set_kernel_timer(gt)
            clip()
            torch.cuda.synchronize()
            ops.set_kernel_timer(None)
        gemm_roof = roofline_gemm(gt.records, 4680 // (world if world > 1 else max(a.emulate_sp, 1)),
                                  (FRAMES // BLOCK) * (len(STEPS_LIST) + 1), model.num_layers, world if world > 1 else max(a.emulate_sp, 1))
    pipe.args.pair_forwards = pair_was
    ks = timer.summary().get("attn_self", dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
    attn_tflops = ks["flops"] / (ks["ms"] * 1e-3) / 1e12 if ks["ms"] else 0.0
    nblk = FRAMES // BLOCK
    for b in range(nblk):
        ms = [s.elapsed_time(e) for (bi, s, e) in evs if bi == b]
        per_block_ms.append(round(sum(ms) / len(ms), 3))
    denoise_ms = [s.elapsed_time(e) for i, (bi, s, e) in enumerate(evs) if i % (len(STEPS_LIST) + 1) != len(STEPS_LIST)]

    if res is None:                      # ranks > 0: their part of the instrumented clips is done
        return False
    res.update({
        "ms_per_denoise_step": round(sum(denoise_ms) / len(denoise_ms), 3),
        "ms_per_forward_by_block": per_block_ms,
        "timed_clip_ms_per_block": {"ms": paired_block_ms, "sum": round(sum(paired_block_ms), 1),
                                    "what": "one more clip exactly as the timed ones (paired forwards as configured, no instrumentation): wall time "
                                            "between block callbacks; with the pairs on a block's re-run overlaps the next block's first step, so "
                                            "`ms_per_denoise_step` x 28 + re-runs (measured with the pairs off) does not add up to `ms_per_step`, this does"},
        "roofline": {"kernel": "ifx::attn_fwd_pp_kernel (block-causal flash attention over the KV manager's view, `ifx_attn_fwd_paged`; self-attention launches)", "bound": "mfma",
                     "achieved": round(attn_tflops, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(attn_tflops / PEAK_BF16_TFLOPS, 4), "traffic": None,
                     "launches": ks["launches"], "avg_launch_ms": round(ks["ms"] / max(ks["launches"], 1), 4),
                     "algorithmic_flops_per_launch": "4*N*L*d, N=4680/n_gpus, d=1536, L=(b+1)*4680",
                     "algorithmic_gbps": round(ks["bytes"] / (ks["ms"] * 1e-3) / 1e9, 1) if ks["ms"] else None,
                     "measured_on": "HIP events around every self-attention launch of ONE clip run right behind the timed region "
                                    "(same process, same launches; kept out of `value`)"},
    })
    if world > 1:
        # the first real multi-GPU line is to be read against a PREDICTION (round-5 verdict, item 6): one emulated rank of `world` on one
        # GPU with the exchange replaced by local copies = this rank's kernels with ZERO wire cost (profiles/sp_emulated_prediction.json,
        # measured by `bench.py --emulate-sp P --sp-exchange peer`).  xGMI can only add to it: measured / predicted >= 1 is expected,
        # and predicted 1-GPU / P-GPU ratios of 1.7 / 2.6 / 3.7 say that >= 4x at 8 GPUs is NOT expected from this decomposition.
        try:
            with open(os.path.join(ROOT, "profiles", "sp_emulated_prediction.json")) as f:
                pred = json.load(f)
            p_ms = pred.get("ms_per_clip", {}).get(f"sp{world}")
            res["sp_prediction"] = {"emulated_rank_ms_per_clip": p_ms, "one_gpu_ms_per_clip_same_box": pred.get("ms_per_clip", {}).get("sp1"),
                                    "measured_over_predicted": round(dt / a.steps * 1e3 / p_ms, 3) if p_ms else None, "source": pred.get("source")}
        except Exception as e:
            res["sp_prediction"] = {"error": f"{type(e).__name__}: {e}"}
    res["roofline"].update(pmc_traffic(world if world > 1 else max(a.emulate_sp, 1)))
    ck = clocks.summary()
    res["roofline"]["clocks"] = ck
    if ck["sclk_mhz_median"]:
        # the dense bf16 peak is 256 CUs x 4 SIMDs x 1024 FLOP/clk at 2.4 GHz; the same pipes at the clock the timed region sustained
        res["roofline"]["frac_at_clock"] = round(attn_tflops / (PEAK_BF16_TFLOPS * ck["sclk_mhz_median"] / 2400.0), 4)
    if gemm_roof:
        res["roofline_gemm"] = gemm_roof
    if breakdown:
        res["kernel_breakdown"] = breakdown
    if world == 1 and not a.no_decode_leg and a.emulate_sp <= 1:
        res["per_block_decode"] = per_block_decode_leg(lambda cb: pipe.inference(
            noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs,
            decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False, block_callback=cb))
        res["vae_decode"] = vae_decode_leg()
    if world == 1 and not a.no_decode_leg and a.emulate_sp <= 1:
        res["text_encoder"] = text_encoder_leg()
    if world == 1 and not a.no_config_legs and a.emulate_sp <= 1 and a.quant == "none" and not a.layers:
        res["quant_fp8"] = quant_leg("fp8", gen, clip, pipe_args=pipe.args)
        res["quant_int8"] = quant_leg("int8", gen, clip, pipe_args=pipe.args)
        kvm.free(reqs[0])
        torch.cuda.empty_cache()
        res["causvid_720p"] = causvid_720p_leg(model, device)
        res["streaming_steady"] = streaming_steady_leg(model, gen, device)
        res["batch2"] = batch_leg(model, gen, device, 2)
        res["magi_cp8_emulated"] = magi_cp8_emulated_leg(device)                          # the named config: fp8_quant
        bf = magi_cp8_emulated_leg(device, fp8_quant=False, breakdown=False)
        res["magi_cp8_emulated"]["bf16_weights"] = {k: bf[k] for k in ("ms_clip_rank", "ms_per_denoise_forward_rank")}
    parity_failed = False
    if world == 1 and not a.no_cpu_baseline:
        run_gpu1 = not a.no_config_legs and a.emulate_sp <= 1 and a.quant == "none" and not a.layers
        res["cpu_baseline"] = cpu_baseline(a.cpu_layers, gpu_leg=(lambda W: config1_gpu(model, gen, device, W)) if run_gpu1 else None)
        if "gpu_same_config" in res["cpu_baseline"]:
            res["config1_gpu"] = res["cpu_baseline"].pop("gpu_same_config")
        par = res["cpu_baseline"].get("parity_vs_gpu")
        parity_failed = par is not None and not par.get("ok", False)
        if parity_failed:
            res["INVALID"] = "config-1 parity check failed: " + json.dumps(par)
    return parity_failed


if __name__ == "__main__":
    main()

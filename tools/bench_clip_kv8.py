"""One full 480p Self-Forcing clip (21 latent frames = 7 blocks x (4 denoise + 1 context) forwards, synthetic Wan2.1-1.3B weights) with
the 8-bit self-attention cache (kv_cache_dtype="fp8_e4m3") against the same clip with the bf16 cache, alternating in one process:
wall time around a device synchronise, median and spread of N clips each, and the rel-L2 between the two clips' latents.
    python tools/bench_clip_kv8.py [--rounds 3] [--layers 30] [--out FILE.json]
`--frame-wise`: INSTEAD, the frame-wise form of the clip (num_frame_per_block = 1: 1560 query rows per forward) with the 8-bit cache,
`kv8_split` on against off (legs `split_off`, `split_on`, `split_off_again` alternating).  `--frame-wise --ring`: the same three legs
on the ring format (kv_cache_dtype="fp8_e4m3_ring", nothing evicted in a clip of 21 frames) with `kv8_ring_split` on against off."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WAN_1_3B = dict(patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=1536, ffn_dim=8960, freq_dim=256, text_dim=4096, out_dim=16,
                num_heads=12, num_layers=30, eps=1e-6)
LATENT, FRAMES, BLOCK, STEPS = (16, 60, 104), 21, 3, [1000, 750, 500, 250]


def build(device, layers, kv_cache_dtype, pe, block=BLOCK, **model_kw):
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    from inferix_amd.wan import HipCausalWanModel, HipWanDiffusionWrapper
    from inferix_amd.wan.synthetic import synthetic_state_dict
    model = HipCausalWanModel(**dict(WAN_1_3B, num_layers=layers), device=device, kv_cache_dtype=kv_cache_dtype, **model_kw)
    model.load_state_dict(synthetic_state_dict(model, seed=0))
    gen = HipWanDiffusionWrapper(model=model, timestep_shift=5.0)
    args = SimpleNamespace(denoising_step_list=STEPS, warp_denoising_step=True, num_frame_per_block=block, independent_first_frame=False,
                           context_noise=0, frame_seq_length=1560, kv_cache_tokens=32760)
    pipe = CausalInferencePipeline(args, device, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
    kvm, reqs = KVCacheManager(device), [KVCacheRequest("clip")]
    noise = torch.randn(1, FRAMES, *LATENT, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(device)
    return lambda: pipe.inference(noise=noise, text_prompts=["synthetic"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                                  decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--frame-wise", action="store_true")
    ap.add_argument("--ring", action="store_true", help="with --frame-wise: the ring format and its kv8_ring_split")
    a = ap.parse_args()
    device = torch.device("cuda")
    torch.set_grad_enabled(False)
    pe = torch.zeros(1, 512, 4096)
    pe[:, :40] = torch.randn(1, 40, 4096, generator=torch.Generator().manual_seed(1))
    pe = pe.to(torch.bfloat16).to(device)
    if a.frame_wise:
        dtype, key = ("fp8_e4m3_ring", "kv8_ring_split") if a.ring else ("fp8_e4m3", "kv8_split")
        off = build(device, a.layers, dtype, pe, block=1, **{key: False})
        clips = {"split_off": off, "split_on": build(device, a.layers, dtype, pe, block=1, **{key: True}), "split_off_again": off}
    else:
        clips = {"bf16": build(device, a.layers, None, pe), "fp8_e4m3": build(device, a.layers, "fp8_e4m3", pe)}
    def run(f):          # the pipeline draws its re-noising eps from the global generator: the same draws for every clip
        torch.manual_seed(3)
        return f()
    outs = {n: run(f) for n, f in clips.items()}           # warm: first use of every launch shape
    torch.cuda.synchronize()
    ms = {n: [] for n in clips}
    for _ in range(a.rounds):
        for n, f in clips.items():                          # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[n] = run(f)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) * 1e3)
    first, second = list(clips)[:2]
    a16, a8 = outs[first].float(), outs[second].float()
    rec = {"layers": a.layers, "kv_cache_dtype": "fp8_e4m3_ring" if a.frame_wise and a.ring else "fp8_e4m3", "forwards_per_clip": (FRAMES // (1 if a.frame_wise else BLOCK)) * (len(STEPS) + 1), "finite": bool(torch.isfinite(a8).all()),
           f"rel_l2_{second}_vs_{first}_latents": float((a8 - a16).norm() / a16.norm())}
    for n, v in ms.items():
        rec[n] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "clips": len(v)}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

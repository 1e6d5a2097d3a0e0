#!/usr/bin/env python3
"""What the glue between two MAGI model forwards costs: `ChunkSchedule.run` (torch operators, a `.item()` per step) against
`ChunkSchedule.walk` (`forward_velocities` + one `ifx_magi_integrate` launch, no host synchronisation), at BASELINE config 5's latent
(16 x 24 x 90 x 90, chunks of 6 frames, window 4, 64 steps: 112 steps per clip), in both guidance modes.

The model is a stub: `forward` returns a preallocated output of the right shape behind a fixed stretch of device work (`--forward-ms`,
a chain of matrix products, so that the queue is as busy as behind a real forward and a host that need not wait can run ahead); the
dispatcher, the three guidance forwards and `forward_velocities` are `HipVideoDiTModel`'s own.  Per step two figures:

  host ms    from the return of a step's last forward to the entry of the next step's first forward, on the host clock: what the host
             spends enqueueing the glue, waits for the device included;
  device ms  between an event recorded behind a step's last forward and one recorded in front of the next step's first forward: how
             long the device goes without model work.

`run`, `walk` and `run` again are interleaved clip by clip in one process; the second `run` is the A/A pair that shows the spread.

    python tools/bench_magi_pipeline.py [--clips 3] [--forward-ms 5] [--steps 64]

`--real` runs another leg instead: `walk` on the real `HipVideoDiTModel` (MAGI-4.5B's dimensions, synthetic weights, `--real-layers` of
them) at the same latent, with the host-side `RangePlan`s and with them withheld (`real_leg`).

    python tools/bench_magi_pipeline.py --real [--real-layers 34] [--clips 3] [--steps 64]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, CW, H, W, CHUNKS, WINDOW = 16, 6, 90, 90, 4, 4


def make_stub(cfg_number: int, forward_ms: float):
    from inferix_amd.magi.model import HipVideoDiTModel

    class Stub:
        forward_dispatcher = HipVideoDiTModel.forward_dispatcher
        _dispatch_3cfg = HipVideoDiTModel._dispatch_3cfg
        forward_3cfg = HipVideoDiTModel.forward_3cfg
        forward_velocities = HipVideoDiTModel.forward_velocities
        generate_kv_range_for_uncondition = HipVideoDiTModel.generate_kv_range_for_uncondition

        def __init__(self):
            self.device = torch.device("cuda", torch.cuda.current_device())
            self.model_config = SimpleNamespace(patch_size=2)
            self.engine_config = SimpleNamespace(shortcut_mode="8,16,16", distill_nearly_clean_chunk_threshold=0.3)
            self.runtime_config = SimpleNamespace(cfg_number=cfg_number, noise2clean_kvrange=[5, 4, 3, 2], clean_chunk_kvrange=1,
                                                  clean_t=0.9999, cfg_t_range=[0.0, 0.0217, 1.0], prev_chunk_scales=[1.5, 1.5, 1.0],
                                                  text_scales=[7.5, 7.5, 0.0])
            self.patch_size, self.t_patch_size = 2, 1
            self.outputs = {}
            self.a = torch.randn(2048, 2048, device=self.device, dtype=torch.bfloat16)
            self.b = torch.empty_like(self.a)
            self.products = 1
            self.stamps = []                        # per forward: (host entry, start event, end event, host exit)
            if forward_ms > 0:                      # size the stretch of device work once
                for _ in range(2):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(64):
                        torch.mm(self.a, self.a, out=self.b)
                    e.record()
                    e.synchronize()
                self.products = max(1, round(forward_ms / (s.elapsed_time(e) / 64)))
            else:
                self.products = 0

        def forward(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None, inference_params=None, **kw):
            t0 = time.perf_counter()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(self.products):
                torch.mm(self.a, self.a, out=self.b)
            key = tuple(x.shape)
            out = self.outputs.get(key)
            if out is None:
                g = torch.Generator(device=self.device).manual_seed(len(self.outputs))
                out = self.outputs[key] = torch.randn(*key, device=self.device, generator=g)
            out = out.clone()                       # the dispatcher blends into what it is handed: keep the stored output as it was
            e.record()
            self.stamps.append((t0, s, e, time.perf_counter()))
            return out

    return Stub()


def one_clip(kind: str, model, sch, x, y, masks, per_step: int):
    model.stamps.clear()
    ip = SimpleNamespace(update_kv_cache=False)
    torch.cuda.synchronize()
    if kind == "run":
        sch.run(model, x, y, masks, ip)
    else:
        for _ in sch.walk(model, x, y, masks, ip):
            pass
    torch.cuda.synchronize()
    st = model.stamps
    assert len(st) == per_step * sch.total_forward_step(), (len(st), per_step, sch.total_forward_step())
    host, dev = [], []
    for k in range(per_step, len(st), per_step):
        last, first = st[k - 1], st[k]
        host.append((first[0] - last[3]) * 1e3)
        dev.append(last[2].elapsed_time(first[1]))
    return host, dev


def real_model(layers: int, device):
    """`HipVideoDiTModel` with MAGI-4.5B's dimensions (bench.py's config 5 model on ONE device, cp_size 1) and synthetic weights; its
    `forward` stamped as the stub's is."""
    from inferix_amd.magi.model import HipVideoDiTModel
    mc = SimpleNamespace(num_layers=layers, hidden_size=3072, ffn_hidden_size=12288, num_attention_heads=24, num_query_groups=8,
                         kv_channels=128, layernorm_epsilon=1e-6, apply_layernorm_1p=True, gated_linear_unit=False,
                         cond_hidden_ratio=0.25, xattn_cond_hidden_ratio=1.0, cond_gating_ratio=1.0, patch_size=2, t_patch_size=1,
                         in_channels=16, out_channels=16, caption_channels=4096, caption_max_length=800, x_rescale_factor=1,
                         half_channel_vae=False)
    ec = SimpleNamespace(cp_size=1, cp_strategy="none", fp8_quant=layers >= 3, kv_offload=False, ulysses_overlap_degree=1, distill=True,
                         shortcut_mode="8,16,16", distill_nearly_clean_chunk_threshold=0.3)
    rc = SimpleNamespace(cfg_number=1, noise2clean_kvrange=[5, 4, 3, 2], clean_chunk_kvrange=1, clean_t=0.9999)
    model = HipVideoDiTModel(SimpleNamespace(model_config=mc, engine_config=ec, runtime_config=rc), device)
    model.load_synthetic(0)
    model.stamps = []
    forward = model.forward

    def stamped(*a, **k):
        t0 = time.perf_counter()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = forward(*a, **k)
        e.record()
        model.stamps.append((t0, s, e, time.perf_counter()))
        return out
    model.forward = stamped
    return model


def real_leg(args, dev):
    """`walk` on the real model, with the host-side `RangePlan`s and with them withheld (the model then reads its ranges back from the
    device at the head of every forward: the behaviour before the plans existed), clip by clip in turn; the second withheld clip is the
    A/A pair.  Per step, besides the two figures of the stub legs (the device gap now counts only the idle stretch BETWEEN two
    forwards; a forward that waits for the device idles it INSIDE, behind its patch embedding):
      step_device_ms   from the end of one forward to the end of the next, on the device: the forward, the glue and every idle stretch
      step_host_ms     from the entry of one forward to the entry of the next, on the host: what it takes to enqueue a step, waits included
    and per clip `lead_ms`, how far the host is ahead when it has enqueued the last step (the wait of the final synchronise)."""
    from inferix_amd.magi.schedule import ChunkSchedule
    from inferix_amd.magi.types import InferenceParams
    sch = ChunkSchedule(args.steps, WINDOW, CHUNKS, CW)
    model = real_model(args.real_layers, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.randn(1, C, CHUNKS * CW, H, W, device=dev, generator=g).repeat(2, 1, 1, 1, 1)
    y = torch.randn(2, CHUNKS, 800, 4096, device=dev, generator=g)
    masks = torch.zeros(2, CHUNKS, 800, device=dev)
    masks[0, :, :100] = 1                                  # a 100-token caption; the null caption row keeps its 2 special tokens
    masks[1, :, :2] = 1
    tokens = CW * (H // 2) * (W // 2)
    names = ("withheld", "plans", "withheld_again")
    res = {k: {"gap_host": [], "gap_dev": [], "step_dev": [], "step_host": [], "lead": [], "clip": []} for k in names}
    finals = {}
    for clip in range(args.clips + 1):
        for name in names:
            x = noise.clone()
            ip = InferenceParams(1, CHUNKS * tokens, device=dev)
            model.stamps.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in sch.walk(model, x, y, masks, ip, host_plans=name == "plans"):
                pass
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            finals[name] = x
            st = model.stamps
            assert len(st) == sch.total_forward_step(), (len(st), sch.total_forward_step())
            if clip == 0:
                continue
            r = res[name]
            for k in range(1, len(st)):
                last, first = st[k - 1], st[k]
                r["gap_host"].append((first[0] - last[3]) * 1e3)
                r["gap_dev"].append(last[2].elapsed_time(first[1]))
                r["step_dev"].append(last[2].elapsed_time(first[2]))
                r["step_host"].append((first[0] - last[0]) * 1e3)
            r["lead"].append((t2 - t1) * 1e3)
            r["clip"].append((t2 - t0) * 1e3)
    out = {"leg": "real model", "layers": args.real_layers, "steps_per_clip": sch.total_forward_step(), "clips": args.clips,
           "plans_equal_withheld": bool(torch.equal(finals["plans"], finals["withheld"]))}
    med = statistics.median
    for name, r in res.items():
        out[name] = {"gap_host_ms_median": round(med(r["gap_host"]), 4), "gap_device_ms_median": round(med(r["gap_dev"]), 4),
                     "step_host_ms_median": round(med(r["step_host"]), 3), "step_device_ms_median": round(med(r["step_dev"]), 3),
                     "step_host_ms_per_clip": round(sum(r["step_host"]) / args.clips, 1),
                     "step_device_ms_per_clip": round(sum(r["step_dev"]) / args.clips, 1),
                     "lead_ms": [round(v, 1) for v in r["lead"]], "clip_ms": [round(v, 1) for v in r["clip"]]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=3, help="clips per variant and guidance mode (the first is a warm-up and is dropped)")
    ap.add_argument("--forward-ms", type=float, default=5.0, help="device work standing in for a model forward (0: none)")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--real", action="store_true", help="the real-model leg only: walk on HipVideoDiTModel with and without host-side plans")
    ap.add_argument("--real-layers", type=int, default=34, help="layers of the real model (fewer: the same head and tail on a shorter forward)")
    args = ap.parse_args()
    from inferix_amd.magi.schedule import ChunkSchedule
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.real:
        return real_leg(args, dev)
    sch = ChunkSchedule(args.steps, WINDOW, CHUNKS, CW)
    y = torch.randn(2, CHUNKS, 8, 16, device=dev)
    masks = torch.ones(2, CHUNKS, 8, device=dev)
    noise = torch.randn(1, C, CHUNKS * CW, H, W, device=dev).repeat(2, 1, 1, 1, 1)
    for cfg_number in (1, 3):
        model = make_stub(cfg_number, args.forward_ms)
        per_step = 1 if cfg_number == 1 else 3
        res = {k: ([], []) for k in ("run", "walk", "run_again")}
        finals = {}
        for clip in range(args.clips + 1):
            for name in ("run", "walk", "run_again"):
                x = noise.clone()
                host, devt = one_clip("walk" if name == "walk" else "run", model, sch, x, y, masks, per_step)
                finals[name] = x
                if clip > 0:
                    res[name][0].extend(host)
                    res[name][1].extend(devt)
        same = bool(torch.equal(finals["run"], finals["walk"]))
        out = {"cfg_number": cfg_number, "steps_per_clip": sch.total_forward_step(), "clips": args.clips, "forward_ms": args.forward_ms,
               "device_products_per_forward": model.products, "walk_equals_run": same}
        for name, (host, devt) in res.items():
            q = statistics.quantiles
            out[name] = {"host_ms_median": round(statistics.median(host), 4), "host_ms_p90": round(q(host, n=10)[8], 4),
                         "device_ms_median": round(statistics.median(devt), 4), "device_ms_p90": round(q(devt, n=10)[8], 4),
                         "host_ms_per_clip": round(sum(host) / args.clips, 2), "device_ms_per_clip": round(sum(devt) / args.clips, 2)}
        print(json.dumps(out))


if __name__ == "__main__":
    main()

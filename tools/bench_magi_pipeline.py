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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=3, help="clips per variant and guidance mode (the first is a warm-up and is dropped)")
    ap.add_argument("--forward-ms", type=float, default=5.0, help="device work standing in for a model forward (0: none)")
    ap.add_argument("--steps", type=int, default=64)
    args = ap.parse_args()
    from inferix_amd.magi.schedule import ChunkSchedule
    dev = torch.device("cuda", torch.cuda.current_device())
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

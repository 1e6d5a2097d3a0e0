#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/magi_walk.npz: what `SampleTransport.integrate_velocity`
(inferix/pipeline/magi/video_generate.py:672-721) hands out behind every forward step of a clip, and the clip it leaves.

The REFERENCE's own `integrate_velocity` (with its `integrate`, `generate_denoise_status_and_sequences` and `try_pad_prefix_video`) runs on
the CPU through oracle/_refstub.py.  The transport object is built without its constructor, as oracle/gen_golden_magi_schedule.py builds
it; the model forward between two integrations is replaced by a seeded velocity, and `x_chunk` is prepared as `forward_velocity` steps
3, 4 and 6 prepare it (the window's frames, the clean chunk in front, the prefix frames pasted over).  Per step the fixture records
whether a chunk is handed out, its index behind the prefix and its frame range; per case the velocities and the final clip.

usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_walk.py
"""
from __future__ import annotations

import os
import sys
from collections import Counter
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refstub  # noqa: E402
from fixture_io import GOLDEN_DIR, save_npz  # noqa: E402
from gen_golden_magi_schedule import load_reference  # noqa: E402

# (num_steps, window_size, chunk_num, chunk_width, prefix frames)
CASES = [
    (8, 4, 3, 2, 0),
    (8, 4, 2, 2, 0),      # fewer chunks than the window
    (4, 1, 3, 2, 0),      # a window of one chunk
    (8, 4, 3, 2, 1),      # image to video: the 1-frame prefix keeps frame 0
    (8, 4, 4, 2, 3),      # one whole chunk plus a frame
    (8, 4, 4, 2, 4),      # whole chunks only: the first handed-out chunk starts exactly at the prefix's end
]
C, H, W = 2, 2, 3


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    vg = load_reference()
    cpu = torch.device("cpu")
    fx = {"n_cases": torch.tensor(len(CASES)), "geom": torch.tensor([C, H, W])}
    for c, (num_steps, window, chunk_num, cw, prefix_frames) in enumerate(CASES):
        g = torch.Generator().manual_seed(1000 + c)
        st = object.__new__(vg.SampleTransport)
        st.chunk_width, st.window_size, st.device = cw, window, cpu
        prefix = None
        if prefix_frames:
            p0 = torch.randn(1, C, prefix_frames, H, W, generator=g)
            prefix = torch.cat([p0, p0], 0)
        st.transport_inputs = [SimpleNamespace(latent_size=(1, C, chunk_num * cw, H, W), num_steps=num_steps, chunk_num=chunk_num,
                                               prefix_video=prefix)]
        x0 = torch.randn(1, C, chunk_num * cw, H, W, generator=g)
        st.xs = [torch.cat([x0, x0], 0)]
        st.ts = [vg.init_t({}, num_steps, cpu, shortcut_mode="")]
        st.chunk_denoise_count, st.x_chunks, st.velocities = [Counter()], [None], [None]
        total = st.total_forward_step(0)
        records, vels = [], []
        for step in range(total):
            (per, stage, idx), (off, cs, ce, ts, te) = st.generate_denoise_status_and_sequences(0, step)
            extra = cs > off and idx == 0
            x_chunk = st.xs[0][:, :, cs * cw: ce * cw].clone()
            if extra:
                x_chunk = torch.cat([st.xs[0][:, :, (cs - 1) * cw: cs * cw].clone(), x_chunk], dim=2)
            if prefix is not None:
                t = torch.zeros(2, x_chunk.size(2) // cw)
                x_chunk, _ = st.try_pad_prefix_video(0, x_chunk, t, prefix_video_start=((cs - 1) if extra else cs) * cw)
            v0 = torch.randn(1, *x_chunk.shape[1:], generator=g)
            st.x_chunks[0], st.velocities[0] = x_chunk, torch.cat([v0, v0], 0)
            vels.append(v0[:, :, cw:].flatten() if extra else v0.flatten())        # the denoising chunks' part: what is integrated
            chunk, index = st.integrate_velocity(0, step)
            if chunk is None:
                records.append([0, -1, -1, -1])
            else:
                # the frame range: the handed-out tensor is a view of the clip that ends with chunk `cs`
                end = (cs + 1) * cw
                start = end - chunk.size(2)
                assert torch.equal(chunk, st.xs[0][0:1, :, start:end])
                records.append([1, int(index), start, end])
        fx[f"c{c}_args"] = torch.tensor([num_steps, window, chunk_num, cw, prefix_frames])
        fx[f"c{c}_hand_out"] = torch.tensor(records)
        fx[f"c{c}_noise"] = x0
        if prefix is not None:
            fx[f"c{c}_prefix"] = prefix[0:1]
        fx[f"c{c}_velocity"] = torch.cat(vels)
        fx[f"c{c}_final"] = st.xs[0][0:1].clone()
        print(c, "steps", total, "handed out", [r[1:] for r in records if r[0]])
    path = os.path.join(GOLDEN_DIR, "magi_walk.npz")
    save_npz(path, fx)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the gated-MLP (SwiGLU, `gated_linear_unit`) layer fixtures of the MAGI-24B configs with the
generator of the ungated ones: oracle/gen_golden_magi_block.py `build(...)` runs the REFERENCE's own `TransformerLayer`
(inferix/models/magi/dit/dit_module.py:1201-1319, fc1 of 2f rows + flashinfer silu_and_mul, :528-549) on the CPU through
oracle/_refstub.py, asserts that oracle/magi_block_oracle.py equals it bit for bit on every output and cache row, and writes
inputs, outputs and cache rows (weights are regenerated from seeds) to tests/golden/:

  magi_block_gated_tiny     : 2 stacked gated layers (hidden 256, ffn 512), the four forwards of magi_block_tiny
  magi_block_gated_fp8_tiny : 3 gated layers under engine_config.fp8_quant, the middle one on the static-scale FP8 linears
  magi_block_24b            : ONE layer at the 24B dimensions (hidden 6144, ffn 16384, 48 q-heads on 8 kv-groups), 2 x 24 tokens

A fixture above the repository's size limit for one file (the 24B one: 48 x 6144 bf16 noise per tensor does not compress) is
stored as `<name>.partK.npz`, whole tensors per part in key order; tests/test_magi_gated_oracle.py `gated_golden` puts them
together again.  The fixture carries no gated flag (`geom` has no slot for it): readers set it with dataclasses.replace.
usage (build container only; the reference tree must exist):  python tools/gen_golden_magi_gated.py
"""
from __future__ import annotations

import dataclasses
import glob
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refstub  # noqa: E402
import gen_golden_magi_block as G  # noqa: E402
import magi_block_oracle as MB  # noqa: E402
from fixture_io import GOLDEN_DIR  # noqa: E402

FILE_LIMIT = 1 << 20              # the repository's limit for one committed file
PART_BYTES = 1000 * 1000          # raw bytes of the arrays of one part: below 1 MiB on disk whatever the compression does


def split_if_large(name: str) -> None:
    """tests/golden/<name>.npz -> <name>.part0.npz ... when the file is larger than one part may be; arrays stay whole."""
    path = os.path.join(GOLDEN_DIR, f"{name}.npz")
    for old in glob.glob(os.path.join(GOLDEN_DIR, f"{name}.part*.npz")):
        os.remove(old)
    if os.path.getsize(path) <= FILE_LIMIT:
        return
    with np.load(path, allow_pickle=False) as z:
        arrays = [(k, z[k]) for k in z.files]
    parts, size = [{}], 0
    for k, a in arrays:
        assert a.nbytes <= PART_BYTES, (k, a.nbytes)
        if size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    for i, part in enumerate(parts):
        p = os.path.join(GOLDEN_DIR, f"{name}.part{i}.npz")
        np.savez_compressed(p, **part)
        print(f"wrote {p} ({os.path.getsize(p)} bytes, {len(part)} arrays)")
    os.remove(path)


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    warnings.filterwarnings("ignore")
    torch.manual_seed(0)
    tiny = dataclasses.replace(MB.tiny_config(), gated_linear_unit=True)
    G.build("magi_block_gated_tiny", tiny, n_layers=2, clip=24, caps=(7, 5), seed=21, wseed=800, n_calls=4)
    G.build("magi_block_gated_fp8_tiny", tiny, n_layers=3, clip=24, caps=(7, 5), seed=23, wseed=900, n_calls=3,
            tap_names=("proj", "mlp"), fp8=True)
    big = MB.MagiLayerConfig(hidden_size=6144, ffn_hidden_size=16384, num_attention_heads=48, num_query_groups=8,
                             gated_linear_unit=True)
    G.build("magi_block_24b", big, n_layers=1, clip=24, caps=(20, 13), seed=22, wseed=1000, n_calls=2, tap_names=("attn_res",))
    for name in ("magi_block_gated_tiny", "magi_block_gated_fp8_tiny", "magi_block_24b"):
        split_if_large(name)


if __name__ == "__main__":
    main()

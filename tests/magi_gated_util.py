"""Shared by the gated-MLP (MAGI-24B) tests: the loader of the fixtures tools/gen_golden_magi_gated.py writes, and the gated config
of a fixture (the fixture's `geom` tensor has no slot for `gated_linear_unit`, so `magi_block_oracle.fixture_geometry` returns the
ungated config: with it, weights and stored outputs disagree at rel-L2 ~0.8)."""
import dataclasses
import glob
import os
import re

import magi_block_oracle as MB
from fixture_io import GOLDEN_DIR, load_npz

GATED_FIXTURES = ("magi_block_gated_tiny", "magi_block_gated_fp8_tiny", "magi_block_24b")


def gated_golden(name: str):
    """tests/golden/<name>.npz, or its parts <name>.partK.npz put together again (a fixture above the size limit for one file)."""
    whole = os.path.join(GOLDEN_DIR, name + ".npz")
    if os.path.exists(whole):
        return load_npz(whole)
    parts = sorted(glob.glob(os.path.join(GOLDEN_DIR, name + ".part*.npz")), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    assert parts, f"no fixture {name}"
    fx = {}
    for p in parts:
        fx.update(load_npz(p))
    return fx


def gated_geometry(fx):
    """`MB.fixture_geometry` with the gated flag set."""
    cfg, n_layers, clip, n_calls, wseed, max_tokens = MB.fixture_geometry(fx)
    return dataclasses.replace(cfg, gated_linear_unit=True), n_layers, clip, n_calls, wseed, max_tokens

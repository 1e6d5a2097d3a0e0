"""The split-key launch of the 8-bit self-attention without a GPU: the plan's arithmetic through ifx_attn_kv8_split_plan, written out
from the rule in include/inferix_hip_kv8_split.h, and the refusals decided on the host."""
import ctypes as C

import pytest

from inferix_amd import _hip

MIN_TILES = 73         # the committed default of attn_kv8_split_min_tiles


def plan(rows, heads, k0, k1, splits=0):
    p = _hip.Kv8SplitPlan()
    assert _hip.load_kv8_split().ifx_attn_kv8_split_plan(rows, heads, k0, k1, splits, C.byref(p)) == _hip.IFX_OK
    return p


def rule(rows, heads, keys, min_tiles=MIN_TILES):
    groups, tiles = -(-rows // 256) * heads, -(-keys // 64)
    if groups > 128:
        return 1
    return max([s for s in range(1, 17) if groups * s <= 256 and tiles // s >= min_tiles], default=1)


@pytest.mark.parametrize("shape,want", [((4680, 12, 0, 32760), 1), ((3120, 12, 0, 32760), 1), ((1560, 12, 0, 32760), 3),
                                        ((1560, 12, 0, 14040), 3),           # 220 tiles: 220 // 3 = 73
                                        ((1560, 12, 0, 9360), 2),            # 147 tiles: 147 // 3 = 49 < 73, 147 // 2 = 73
                                        ((1560, 12, 0, 4680), 1),            # 74 tiles: 74 // 2 = 37 < 73
                                        ((1560, 12, 0, 64 * 8 * 2 - 1), 1),  # 16 tiles
                                        ((256, 12, 0, 32760), 7),            # 12 groups: 512 // 8 = 64 < 73, 512 // 7 = 73
                                        ((72, 2, 0, 21 * 24), 1)])           # the tiny rollout's longest forward: 8 tiles
def test_chooser(shape, want):
    v = C.c_int32(0)
    assert _hip.load().ifx_get_option(b"attn_kv8_split_min_tiles", C.byref(v)) == _hip.IFX_OK and v.value == MIN_TILES
    assert plan(*shape).chunks == want == rule(shape[0], shape[1], shape[3] - shape[2])


@pytest.mark.parametrize("tiles", range(1, 41))
def test_chunks_and_workspace(tiles):
    rows, heads, k0 = 300, 3, 70
    keys, groups = 64 * tiles - 5, 2 * heads
    for splits in range(1, 17):
        p = plan(rows, heads, k0, k0 + keys, splits)
        per = list(p.tiles_per_chunk)
        assert p.chunks == min(splits, tiles) and p.key_tiles == tiles and p.row_tiles == 2
        assert sum(per[:p.chunks]) == tiles and min(per[:p.chunks]) >= 1 and max(per[:p.chunks]) - min(per[:p.chunks]) <= 1 and not any(per[p.chunks:])
        assert sum(p.xcd_groups) == groups and p.lds_bytes == 3 * (64 * 128 + 128 * 64 + 32 * 16)
        if p.chunks == 1:
            assert p.workspace_bytes == p.counter_bytes == 0 and p.grid == 8 * -(-groups // 8)
        else:
            assert p.counter_bytes == 256 and p.workspace_bytes == 256 + p.chunks * heads * 2 * 256 * 132 * 4 and p.grid == 8 * -(-groups // 8) * p.chunks
            assert p.grid // 8 >= max(p.xcd_groups) * p.chunks


def test_refusals():
    lib, p = _hip.load_kv8_split(), _hip.Kv8SplitPlan()
    for bad in [(8, 2, 0, 64, 17), (8, 2, 0, 64, -1), (0, 2, 0, 64, 0), (8, 2, 64, 64, 2)]:
        assert lib.ifx_attn_kv8_split_plan(*bad, C.byref(p)) == _hip.IFX_EINVAL
    # q_rows = 0: everything is checked, then IFX_OK without a launch, so the made-up addresses are never used
    call = lambda splits=2, heads=2, k1=128, ldq=0, rows=0, ws=None, ws_bytes=0: lib.ifx_attn_fwd_kv8_split(
        4096, ldq, 4096, 0, None, 4096, 8192, 12288, 128, 2, rows, heads, 0, k1, splits, ws, ws_bytes, None)
    assert call() == _hip.IFX_OK
    assert call(splits=17) == _hip.IFX_EINVAL and b"num_splits" in lib.ifx_last_error() and call(splits=0) == _hip.IFX_EINVAL
    assert call(heads=3) == _hip.IFX_EINVAL and call(k1=129) == _hip.IFX_EINVAL and call(ldq=200) == _hip.IFX_EINVAL
    # with rows and two chunks the workspace is checked, still ahead of any launch: missing, too small, misaligned
    need = plan(8, 2, 0, 128, 2).workspace_bytes
    assert need == 256 + 2 * 2 * 256 * 132 * 4
    assert call(rows=8) == _hip.IFX_EINVAL and b"workspace" in lib.ifx_last_error()
    assert call(rows=8, ws=4096, ws_bytes=need - 1) == _hip.IFX_EINVAL and call(rows=8, ws=4100, ws_bytes=need + 16) == _hip.IFX_EINVAL
    assert set(_hip.KV8_SPLIT_SIGNATURES) == {"ifx_attn_kv8_split_plan", "ifx_attn_fwd_kv8_split"} and not set(_hip.KV8_SPLIT_SIGNATURES) & set(_hip.SIGNATURES)

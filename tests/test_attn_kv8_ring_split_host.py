"""The grouped split-key launch of the 8-bit ring cache without a GPU: ifx_attn_kv8_grouped_split_plan against the rule in
include/inferix_hip_kv8_ring_split.h written out, the refusals decided on the host and the option's round trip."""
import ctypes as C

import pytest

from inferix_amd import _hip, hip_ops

MIN_TILES = 62         # the committed default of attn_kv8_grouped_split_min_tiles


def plan(rows, heads, G, keys, splits=0):
    p = _hip.Kv8GroupedSplitPlan()
    assert _hip.load_kv8_ring_split().ifx_attn_kv8_grouped_split_plan(rows, heads, G, keys, splits, C.byref(p)) == _hip.IFX_OK
    return p


def walk(G, keys):          # (group, tile in group) of every tile of the grouped walk, in order
    return [(g, j) for g in range(-(-keys // G)) for j in range(-(-min(G, keys - g * G) // 64))]


def rule(rows, heads, G, keys, min_tiles=MIN_TILES):
    groups, tiles = -(-rows // 256) * heads, len(walk(G, keys))
    return max([s for s in range(1, 17) if groups <= 128 and tiles // s >= min_tiles and -(-groups // 8) * s <= 32], default=1)


#                                        shape, chunks at the default, chunks at min_tiles 73
@pytest.mark.parametrize("shape,want,want73", [((1560, 12, 1560, 32760), 2, 2),     # 84 groups: 3 x 11 = 33 workgroups on an XCD of 32
                                               ((1560, 12, 1560, 14040), 2, 2),     # 225 tiles
                                               ((1560, 12, 1560, 7800), 2, 1),      # 125 tiles: 125 // 2 = 62
                                               ((1560, 12, 1560, 4680), 1, 1),      # 75 tiles: 75 // 2 = 37
                                               ((4680, 12, 1560, 32760), 1, 1),     # 228 groups > 128
                                               ((256, 12, 1560, 32760), 8, 7),      # 12 groups, 525 tiles: 525 // 8 = 65, 525 // 7 = 75
                                               ((72, 2, 24, 6 * 24), 1, 1)])        # the tiny ring rollout's window: 6 tiles
def test_chooser(shape, want, want73):
    assert hip_ops.get_option("attn_kv8_grouped_split_min_tiles") == MIN_TILES
    assert plan(*shape).chunks == want == rule(*shape)
    for mt, chunks in ((73, want73), (1, rule(*shape, min_tiles=1))):        # the option's round trip; at 1 the XCD bound alone is left
        with hip_ops.option_scope("attn_kv8_grouped_split_min_tiles", mt):
            assert hip_ops.get_option("attn_kv8_grouped_split_min_tiles") == mt and hip_ops.get_option("attn_kv8_split_min_tiles") == 73
            assert hip_ops.attention_kv8_grouped_split_plan(*shape)["chunks"] == chunks == rule(*shape, min_tiles=mt)
    assert hip_ops.get_option("attn_kv8_grouped_split_min_tiles") == MIN_TILES and plan(*shape).chunks == want


@pytest.mark.parametrize("G,keys", [(24, 72), (100, 300), (128, 448), (64, 1025), (1560, 4680), (1560, 32760), (130, 131)])
def test_chunks_cursors_and_workspace(G, keys):
    rows, heads, groups, tiles = 300, 3, 6, walk(G, keys)
    for splits in range(1, 17):
        p = plan(rows, heads, G, keys, splits)
        n, per = p.chunks, list(p.tiles_per_chunk)
        assert n == min(splits, len(tiles)) and p.key_tiles == len(tiles) and p.tiles_per_group == -(-G // 64) and p.row_tiles == 2 and p.key_groups == -(-keys // G)
        assert sum(per[:n]) == len(tiles) and min(per[:n]) >= 1 and per[:n] == sorted(per[:n], reverse=True) and per[0] - per[n - 1] <= 1
        assert list(zip(p.first_group, p.first_tile))[:n] == [tiles[sum(per[:c])] for c in range(n)] and list(p.last_group)[:n] == [tiles[sum(per[:c + 1]) - 1][0] for c in range(n)]
        assert not any(per[n:] + list(p.first_group)[n:] + list(p.first_tile)[n:] + list(p.last_group)[n:])
        assert sum(p.xcd_groups) == groups and p.lds_bytes == 3 * (64 * 128 + 128 * 64 + 32 * 16)
        assert p.grid == 8 * -(-groups // 8) * n and p.grid // 8 >= max(p.xcd_groups) * n
        assert (p.counter_bytes, p.workspace_bytes) == ((0, 0) if n == 1 else (256, 256 + n * heads * 2 * 256 * _hip.IFX_KV8_SPLIT_ROW_WORDS * 4))


def test_refusals():
    lib, p = _hip.load_kv8_ring_split(), _hip.Kv8GroupedSplitPlan()
    for bad in [(8, 2, 64, 64, 17), (8, 2, 64, 64, -1), (0, 2, 64, 64, 0), (8, 2, 0, 64, 2), (8, 2, 64, 0, 2), (8, 0, 64, 64, 2)]:
        assert lib.ifx_attn_kv8_grouped_split_plan(*bad, C.byref(p)) == lib.ifx_attn_kv8_grouped_split_plan(8, 2, 64, 64, 2, None) == _hip.IFX_EINVAL
    # q_rows = 0: everything is checked, then IFX_OK without a launch, so the made-up addresses are never used
    call = lambda splits=2, heads=2, keys=128, ldq=0, rows=0, G=64, slots=128, ws=None, ws_bytes=0: lib.ifx_attn_fwd_kv8_grouped_split(
        4096, ldq, 4096, 0, None, 4096, 8192, 12288, slots, 2, G, rows, heads, keys, splits, ws, ws_bytes, None)
    assert call() == _hip.IFX_OK
    assert call(splits=17) == _hip.IFX_EINVAL and b"num_splits" in lib.ifx_last_error() and call(splits=0) == _hip.IFX_EINVAL
    assert call(heads=3) == _hip.IFX_EINVAL and call(keys=129) == _hip.IFX_EINVAL and call(keys=0) == _hip.IFX_EINVAL and call(ldq=200) == _hip.IFX_EINVAL
    assert call(G=0) == _hip.IFX_EINVAL and call(G=48) == _hip.IFX_EINVAL           # 128 slots are no whole number of groups of 48
    # with rows and two chunks the workspace is checked, still ahead of any launch: missing, too small, misaligned
    need = plan(8, 2, 64, 128, 2).workspace_bytes
    assert call(rows=8) == _hip.IFX_EINVAL and b"workspace" in lib.ifx_last_error()
    assert call(rows=8, ws=4096, ws_bytes=need - 1) == _hip.IFX_EINVAL and call(rows=8, ws=4100, ws_bytes=need + 16) == _hip.IFX_EINVAL
    assert set(_hip.KV8_RING_SPLIT_SIGNATURES) == {"ifx_attn_kv8_grouped_split_plan", "ifx_attn_fwd_kv8_grouped_split"} and not set(_hip.KV8_RING_SPLIT_SIGNATURES) & set(_hip.SIGNATURES)

"""ifx_attn_kv8_ranges_plan (include/inferix_hip_kv8_magi.h) through the C ABI, no GPU: every (range, head, row tile) exactly once, a
stream on one XCD, the balance bound, the refusals."""
import ctypes as C

import pytest

from inferix_amd import _hip

OK, EINVAL, EUNSUP = 0, _hip.IFX_EINVAL, _hip.IFX_EUNSUP


def plan(q_ranges, k_ranges, heads, kv_heads, seg_split, capacity=None):
    lib = _hip.load_kv8_magi()
    n = len(q_ranges)
    qa = (C.c_int32 * (2 * n))(*[v for r in q_ranges for v in r])
    ka = (C.c_int32 * (2 * n))(*[v for r in k_ranges for v in r])
    cap = n * kv_heads if capacity is None else capacity
    p, sr, sh, st = _hip.Kv8RangesPlan(), (C.c_int32 * max(cap, 1))(), (C.c_int32 * max(cap, 1))(), (C.c_int32 * max(cap, 1))()
    rc = lib.ifx_attn_kv8_ranges_plan(qa, ka, n, heads, kv_heads, seg_split, C.byref(p), sr, sh, st, cap)
    return rc, p, sr, sh, st


# MAGI-4.5B mid-clip (24 / 8 heads, 4 chunks in flight), one cp = 8 rank's share (3 / 1), a ragged set with an empty query range
SETS = [([(0, 4050), (4050, 8100), (8100, 12150), (12150, 16200)], [(0, 20250), (0, 24300), (0, 28350), (0, 32400)], 24, 8, 28350),
        ([(0, 4050), (4050, 8100)], [(0, 8100), (0, 12150)], 3, 1, 0),
        ([(0, 70), (73, 373), (376, 376), (400, 1000)], [(0, 64), (100, 300), (0, 449), (100, 549)], 6, 2, 150)]


@pytest.mark.parametrize("q_ranges,k_ranges,heads,kv_heads,seg_split", SETS)
def test_plan_invariants(q_ranges, k_ranges, heads, kv_heads, seg_split):
    rc, p, sr, sh, st = plan(q_ranges, k_ranges, heads, kv_heads, seg_split)
    assert rc == OK
    group = heads // kv_heads
    row_tiles = [-(-(e - s) // 256) for s, e in q_ranges]
    key_tiles = []
    for s, e in k_ranges:      # the cut walk: tiles up to seg_split, then tiles from it
        a, b = (max(0, min(e, seg_split) - s), max(0, e - max(s, seg_split))) if seg_split else (e - s, 0)
        key_tiles.append(-(-a // 64) + -(-b // 64))
    assert list(p.key_tiles[:len(k_ranges)]) == key_tiles
    units, cost, largest = [], [0] * 8, 0
    for x in range(8):
        t = 0
        for s in range(p.xcd_first[x], p.xcd_first[x + 1]):      # a stream's tiles are consecutive local tiles of ONE XCD
            assert st[s] == t
            r = sr[s]
            units += [(r, sh[s] * group + g, tile) for g in range(group) for tile in range(row_tiles[r])]
            t += group * row_tiles[r]
            cost[x] += group * row_tiles[r] * key_tiles[r]
            largest = max(largest, group * row_tiles[r] * key_tiles[r])
        assert t == p.xcd_tiles[x] and cost[x] == p.xcd_cost[x]
    want = [(r, h, tile) for r in range(len(q_ranges)) for h in range(heads) for tile in range(row_tiles[r])]
    assert sorted(units) == want                                   # every (range, head, row tile) exactly once
    assert p.n_streams == p.xcd_first[8] == sum(1 for t in row_tiles if t) * kv_heads
    assert p.grid == 8 * max(p.xcd_tiles) and max(cost) <= sum(cost) / 8 + largest
    assert p.arg_bytes <= 4096 and p.lds_bytes == 3 * (64 * 128 + 128 * 64 + 32 * 16)


@pytest.mark.parametrize("args,code,words", [
    (([(0, 8)] * 9, [(0, 8)] * 9, 2, 2, 0), EUNSUP, b"range by range"),              # n_ranges > 8
    (([(0, 8)] * 8, [(0, 8)] * 8, 34, 17, 0), EUNSUP, b"range by range"),            # 136 streams > 128
    (([(0, 8)], [(0, 8)], 3, 2, 0), EINVAL, b"kv_heads"),                            # heads % kv_heads
    (([(8, 0)], [(0, 8)], 2, 2, 0), EINVAL, b"query ranges"),                        # reversed query range
    (([(0, 8)], [(5, 5)], 2, 2, 0), EINVAL, b"key ranges"),                          # empty key range
    (([(0, 8)], [(0, 8)], 2, 2, -1), EINVAL, b"seg_split"),
    (([(0, 8), (8, 16)], [(0, 8), (0, 8)], 2, 2, 0, 3), EINVAL, b"room for 3")])     # capacity too small
def test_plan_refusals(args, code, words):
    rc = plan(*args)[0]
    msg = _hip.load().ifx_last_error()
    assert rc == code and b"ifx_attn_kv8_ranges_plan" in msg and words in msg, (rc, msg)

"""The ring cache's multi-session attention launch without a GPU (include/inferix_hip_kv8_ring_sessions.h): its work split counts a
stream's key tiles as the grouped launch walks them."""
import pytest

from inferix_amd import _hip

EIGHT_SAMPLES = [(4680, 4680 + 4680 * i) for i in (3, 0, 5, 1, 6, 2, 6, 4)]
#       items (rows, kv_len), heads, G
SETS = [([(1, 100), (65, 300), (300, 250), (0, 100)], 4, 100), ([(300, 200), (33, 63), (300, 1000)], 2, 24), (EIGHT_SAMPLES, 12, 1560),
        ([(1, 100), (65, 300), (300, 250), (0, 100)], 4, 64)]


def _costs(items, heads, G):
    from inferix_amd import hip_ops as ops
    p = ops.attention_kv8_grouped_multi_plan(items, heads, G)
    single = [ops.attention_kv8_grouped_plan(r, heads, G, k) if r else dict(row_tiles=0, key_tiles=0) for r, k in items]
    return p, [s["row_tiles"] for s in single], [s["key_tiles"] for s in single]


@pytest.mark.parametrize("items,heads,G", SETS, ids=lambda v: str(v) if isinstance(v, int) else f"{len(v)}items")
def test_grouped_multi_plan(items, heads, G):
    p, rt, kt = _costs(items, heads, G)
    assert kt == [(k // G) * -(-G // 64) + -(-(k % G) // 64) if r else 0 for r, k in items]
    n = p["n_streams"]
    assert n == heads * sum(r > 0 for r in rt) and p["xcd_first"][0] == 0 and p["xcd_first"][8] == n
    assert sorted(zip(p["stream_item"], p["stream_head"])) == [(i, h) for i in range(len(items)) if rt[i] for h in range(heads)]
    for x in range(8):
        mine = p["stream_item"][p["xcd_first"][x]:p["xcd_first"][x + 1]]
        assert p["xcd_cost"][x] == sum(rt[i] * kt[i] for i in mine) and p["xcd_tiles"][x] == sum(rt[i] for i in mine)
        assert [kt[i] for i in mine] == sorted((kt[i] for i in mine), reverse=True)          # longest walk first
    assert max(p["xcd_cost"]) <= sum(p["xcd_cost"]) / 8 + max(r * k for r, k in zip(rt, kt))
    assert p["grid"] == 8 * max(p["xcd_tiles"]) and p["arg_bytes"] <= 4096


def test_cost_counts_grouped_tiles_and_the_table_has_an_end():
    """The same set with G = 64 (whole tiles: the flat count) and G = 100 (two tiles per group, the second partial)."""
    (p64, _, kt64), (p100, _, kt100) = _costs(*SETS[3]), _costs(*SETS[0])
    assert kt64 == [2, 5, 4, 0] and kt100 == [2, 6, 5, 0] and sorted(p64["xcd_cost"]) != sorted(p100["xcd_cost"])
    from inferix_amd import hip_ops as ops
    assert ops.attention_kv8_grouped_multi_plan([(8, 8)] * 8, 40, 8)["n_streams"] == 320
    with pytest.raises(_hip.HipKernelError, match=rf"code {_hip.IFX_EUNSUP}\)"):
        ops.attention_kv8_grouped_multi_plan([(8, 8)] * 8, 41, 8)
    # the launcher, decided on the host: items without rows are checked and skipped, so the made-up addresses are never used
    lib = _hip.load_kv8_ring_sessions()
    item = lambda **kw: _hip.AttnKv8GroupedItem(**{**dict(q8=4096, ldq=0, ldo=0, out=4096, k=8192, v=12288, v_scale=16384, num_slots=64, q_rows=0, kv_len=64), **kw})
    call = lambda its, heads=2, G=8: lib.ifx_attn_fwd_kv8_grouped_multi((_hip.AttnKv8GroupedItem * len(its))(*its), len(its), heads, heads, G, None)
    assert call([item()] * 8) == _hip.IFX_OK and call([item()] * 9) == _hip.IFX_EINVAL
    for bad in (dict(kv_len=65), dict(num_slots=60), dict(ldq=200), dict(v_scale=0), dict(q_rows=-1)):
        assert call([item(), item(**bad)]) == _hip.IFX_EINVAL and b"item 1" in lib.ifx_last_error(), bad
    assert call([item()] * 8, heads=41) == _hip.IFX_EUNSUP and b"raster table" in lib.ifx_last_error()

"""The 8-bit cache's multi-session entry points without a GPU: the work split of the attention launch, the refusals decided on the
host, and the fourth header's derived bindings against the C compiler."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from inferix_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING, SLOT = 3, 64 * 128 + 128 * 64 + 32 * 16
EIGHT = [(1, 0, 1), (33, 0, 63), (256, 0, 64), (300, 0, 65), (33, 0, 200), (300, 0, 200), (33, 70, 270), (256, 0, 1)]
#       items (rows, kv_start, kv_len), heads
SETS = [([(300, 0, 200)], 2), ([(33, 0, 1), (300, 0, 64 * (RING + 2) + 5)], 4), (EIGHT, 4), (EIGHT, 2), ([(300, 0, 200), (300, 0, 200), (33, 0, 63)], 2),
        ([(300, 0, 200), (0, 0, 8), (33, 70, 270)], 4), ([(4680, 0, 4680 + 4011 * i) for i in (3, 0, 5, 1, 7, 2, 6, 4)], 12),
        ([(1560, 0, 1560)] * 8, 40)]


@pytest.mark.parametrize("items,heads", SETS, ids=lambda v: str(v) if isinstance(v, int) else f"{len(v)}items")
def test_plan(items, heads):
    from inferix_amd import hip_ops as ops
    p = ops.attention_kv8_multi_plan(items, heads)
    rt, kt = [-(-r // 256) for r, _, _ in items], [-(-(k1 - k0) // 64) for _, k0, k1 in items]
    n = p["n_streams"]
    assert n == heads * sum(r > 0 for r in rt) and p["xcd_first"][0] == 0 and p["xcd_first"][8] == n
    assert sorted(p["order"]) == list(range(len(items)))
    keys = [items[i][2] - items[i][1] for i in p["order"]]
    assert keys == sorted(keys, reverse=True)
    # workgroup b: XCD b & 7, local tile b >> 3; every (item, head, row tile) exactly once, all tiles of a stream on one XCD
    ran, cost = [], [0] * 8
    for b in range(p["grid"]):
        x, lt = b & 7, b >> 3
        if lt >= p["xcd_tiles"][x]:
            continue
        s = max(s for s in range(p["xcd_first"][x], p["xcd_first"][x + 1]) if p["stream_tile0"][s] <= lt)
        ran.append((p["stream_item"][s], p["stream_head"][s], lt - p["stream_tile0"][s]))
    assert sorted(ran) == sorted((i, h, t) for i in range(len(items)) for h in range(heads) for t in range(rt[i]))
    assert len(set(zip(p["stream_item"], p["stream_head"]))) == n
    for x in range(8):
        mine = p["stream_item"][p["xcd_first"][x]:p["xcd_first"][x + 1]]
        assert [kt[i] for i in mine] == sorted((kt[i] for i in mine), reverse=True)          # longest key range first
        cost[x] = sum(rt[i] * kt[i] for i in mine)
        assert p["xcd_tiles"][x] == sum(rt[i] for i in mine)
    assert cost == p["xcd_cost"] and max(cost) <= sum(cost) / 8 + max(r * k for r, k in zip(rt, kt))
    assert p["grid"] == 8 * max(p["xcd_tiles"]) and p["lds_bytes"] == RING * SLOT and p["arg_bytes"] <= 4096


def test_refusals():
    """Decided on the host: q_rows = 0 items are checked and skipped, so the made-up addresses are never used."""
    lib = _hip.load_kv8_sessions()
    item = lambda **kw: _hip.AttnKv8Item(**{**dict(q8=4096, ldq=0, ldo=0, out=4096, k=8192, v=12288, v_scale=16384, num_slots=64, q_rows=0,
                                                    kv_start=0, kv_len=64), **kw})
    call = lambda its, heads=2, kvh=2: lib.ifx_attn_fwd_kv8_multi((_hip.AttnKv8Item * max(len(its), 1))(*its), len(its), heads, kvh, None)
    assert call([item()] * 8) == _hip.IFX_OK
    assert call([]) == _hip.IFX_EINVAL and call([item()] * 9) == _hip.IFX_EINVAL and b"1..8 items" in lib.ifx_last_error()
    assert call([item()], heads=3) == _hip.IFX_EINVAL and b"no multiple of kv_heads" in lib.ifx_last_error()
    for bad in (dict(kv_len=65), dict(kv_start=64), dict(ldq=200), dict(ldq=264), dict(q8=4100), dict(ldo=260), dict(out=0), dict(v_scale=0), dict(q_rows=-1)):
        assert call([item(), item(**bad)]) == _hip.IFX_EINVAL and b"item 1" in lib.ifx_last_error(), bad
    assert call([item(num_slots=1 << 23)]) == _hip.IFX_EUNSUP and b"2 GiB" in lib.ifx_last_error()
    assert call([item()] * 8, heads=40, kvh=40) == _hip.IFX_OK          # the table's size: 8 items x 40 heads
    assert call([item()] * 8, heads=41, kvh=41) == _hip.IFX_EUNSUP and b"raster table" in lib.ifx_last_error()
    plan, arr = _hip.Kv8MultiPlan(), lambda *v: (C.c_int32 * 8)(*v)
    cap = (C.c_int32 * 512)()
    pl = lambda rows, k0, k1, n, heads, room=512: lib.ifx_attn_kv8_multi_plan(arr(*rows), arr(*k0), arr(*k1), n, heads, C.byref(plan), cap, cap, cap, room)
    assert pl([8], [0], [8], 1, 2) == _hip.IFX_OK and pl([8], [0], [8], 1, 2, room=1) == _hip.IFX_EINVAL
    for bad in (([8], [0], [8], 0, 2), ([8] * 8, [0] * 8, [8] * 8, 9, 2), ([8], [0], [8], 1, 0), ([-1], [0], [8], 1, 2), ([8], [-1], [8], 1, 2), ([8], [8], [8], 1, 2)):
        assert pl(*bad) == _hip.IFX_EINVAL, bad
    assert pl([8] * 8, [0] * 8, [8] * 8, 8, 41) == _hip.IFX_EUNSUP
    # the append: per item what the single call refuses
    rope = _hip.RopeGrid(4096, 1024, 0, 4, 6, 0, 24, 1.0, 0)
    app = lambda **kw: _hip.Kv8AppendItem(**{**dict(qkv=4096, q8_out=4096, rope=C.pointer(rope), k=8192, v=12288, v_scale=16384, qkv_row_stride=768,
                                                    num_slots=64, local_start=0, rows=0), **kw})
    acall = lambda its, kvh=2, hd=128, dim=256: lib.ifx_rmsnorm_rope_kv8_append_multi((_hip.Kv8AppendItem * max(len(its), 1))(*its), len(its), 4096, 4096,
                                                                                     kvh, hd, dim, 1e-6, None)
    assert acall([app()] * 8) == _hip.IFX_OK
    assert acall([]) == _hip.IFX_EINVAL and acall([app()] * 9) == _hip.IFX_EINVAL and acall([app()], kvh=3) == _hip.IFX_EINVAL
    for bad in (dict(local_start=65), dict(local_start=-1), dict(qkv_row_stride=760), dict(qkv_row_stride=772), dict(rope=None), dict(k=0), dict(rows=-1)):
        assert acall([app(), app(**bad)]) == _hip.IFX_EINVAL and b"item 1" in lib.ifx_last_error(), bad
    assert acall([app()], kvh=4, hd=64) == _hip.IFX_EUNSUP and b"head_dim 64" in lib.ifx_last_error()
    assert acall([app()], kvh=32, hd=128, dim=4096) == _hip.IFX_EINVAL          # qkv_row_stride no longer covers 3 x dim


def test_kv8_sessions_header(tmp_path):
    """A table of its own, disjoint from the other three; struct layouts equal the C compiler's."""
    abi = _hip._KV8_SESSIONS_ABI
    assert set(abi.functions) == {"ifx_attn_fwd_kv8_multi", "ifx_attn_kv8_multi_plan", "ifx_rmsnorm_rope_kv8_append_multi"}
    assert not set(abi.functions) & (set(_hip.SIGNATURES) | set(_hip.SESSIONS_SIGNATURES) | set(_hip.KV8_SIGNATURES))
    assert abi.constants == {"IFX_KV8_MULTI_MAX_ITEMS": 8, "IFX_KV8_MULTI_MAX_STREAMS": 320}
    assert dict(_hip.Kv8AppendItem._fields_)["rope"] is C.POINTER(_hip.RopeGrid)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not present")
    lines, derived = ['#include <stddef.h>', '#include <stdio.h>', '#include "inferix_hip_kv8_sessions.h"', "int main(void) {"], {}
    for name, cls in abi.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        derived[name] = C.sizeof(cls)
        for f, _ in cls._fields_:
            lines.append(f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
            derived[f"{name}.{f}"] = getattr(cls, f).offset
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    b = subprocess.run([hipcc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    compiled = {k: int(v) for k, v in (line.split() for line in p.stdout.splitlines())}
    assert len(derived) == 3 + 11 + 10 + 8 and derived == compiled

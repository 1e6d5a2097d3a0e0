"""Shared by tests/test_hip_attn_multi.py (gpu) and tests/test_attn_multi_host.py: raw calls of ifx_attn_fwd_multi and the argument
refusals of the entry point, which are decided on the host before anything is launched (the pointers are never followed)."""
import ctypes as C

FAKE = 0x10000          # a non-null "device pointer": the refusals below return before a launch


def raw_items(lib_mod, specs):
    """specs: dicts with q, out (ints), view (KvView struct), q_rows, kv_start, kv_len, optional ldq / ldo -> (array, keep-alive)."""
    arr = (lib_mod.AttnItem * max(1, len(specs)))()
    keep = []
    for a, s in zip(arr, specs):
        keep.append(s["view"])
        a.q, a.out, a.ldq, a.ldo = s.get("q", FAKE), s.get("out", FAKE), s.get("ldq", 0), s.get("ldo", 0)
        a.kv = C.pointer(s["view"])
        a.q_rows, a.kv_start, a.kv_len = s.get("q_rows", 64), s.get("kv_start", 0), s.get("kv_len", 100)
    return arr, keep


def fake_view(lib_mod, *, table=False, page_size=1, slots=4096, kv_heads=12, head_dim=128, seg_split=0, seg_delta=0):
    return lib_mod.KvView(FAKE, FAKE, FAKE if table else None, page_size, slots, kv_heads, head_dim, seg_split, seg_delta)


def refusal_cases(lib_mod):
    """name -> (specs, n_items or None, heads, expected code, fragment of the message)"""
    v = lambda **kw: fake_view(lib_mod, **kw)
    one = lambda view, **kw: dict(view=view, **kw)
    return {
        "no items": ([one(v())], 0, 12, -1, "1..8 items per launch (got 0)"),
        "nine items": ([one(v()) for _ in range(9)], 9, 12, -1, "1..8 items per launch (got 9)"),
        "null q": ([one(v(), q=None)], None, 12, -1, "null argument in item 0"),
        "head_dim 64": ([one(v(head_dim=64))], None, 12, -1, "head_dim 64 not built"),
        "heads 5 on 2": ([one(v(kv_heads=2))], None, 5, -1, "heads 5 is not a multiple of kv_heads 2"),
        "differing kv_heads": ([one(v(kv_heads=12)), one(v(kv_heads=6))], None, 12, -1, "item 1 has kv_heads 6, item 0 has 12"),
        "key range past the slots": ([one(v(slots=100), kv_len=101)], None, 12, -1, "key range [0, 101) out of range (capacity 100)"),
        "no rows": ([one(v(), q_rows=0)], None, 12, -1, "item 0: 0 rows"),
        "short stride": ([one(v(), ldq=1528)], None, 12, -1, "row strides (1528, 1536) of item 0"),
        "two-segment view": ([one(v(seg_split=50, seg_delta=8))], None, 12, -3, "item 0 is a two-segment view (seg_split 50)"),
        "two-row pages": ([one(v(table=True, page_size=2))], None, 12, -3, "item 0 needs per-lane page translation (page_size 2)"),
        "one-row pages": ([one(v()), one(v(table=True, page_size=1))], None, 12, -3, "per-lane page translation (page_size 1)"),
        "mixed kinds": ([one(v()), one(v(table=True, page_size=64))], None, 12, -3, "item 1 is paged and item 0 is not"),
    }


def check_refusals(lib_mod, variant_setter):
    lib = lib_mod.load_sessions()
    variant_setter(7)                        # (under the automatic choice small items are refused first: see "auto" below)
    for name, (specs, n, heads, code, text) in refusal_cases(lib_mod).items():
        arr, keep = raw_items(lib_mod, specs)
        rc = lib.ifx_attn_fwd_multi(arr, len(specs) if n is None else n, heads, 0.0, None)
        msg = lib.ifx_last_error().decode()
        assert rc == code and text in msg and msg.startswith("ifx_attn_fwd_multi"), (name, rc, msg)
    assert lib.ifx_attn_fwd_multi(None, 1, 12, 0.0, None) == -1 and b"ifx_attn_fwd_multi: null argument" in lib.ifx_last_error()
    # schedules the multi kernels are not built for, and the four-wave-kernel launches of the automatic choice: IFX_EUNSUP, no launch
    arr, keep = raw_items(lib_mod, [dict(view=fake_view(lib_mod), q_rows=2048, kv_len=4000)] * 2)
    for variant in (1, 2, 3, 4, 5):
        variant_setter(variant)
        assert lib.ifx_attn_fwd_multi(arr, 2, 12, 0.0, None) == -3 and b"attn_variant 6 and 7" in lib.ifx_last_error(), variant
    variant_setter(0)
    small, keep2 = raw_items(lib_mod, [dict(view=fake_view(lib_mod), q_rows=2048, kv_len=4000), dict(view=fake_view(lib_mod), q_rows=300, kv_len=4000)])
    assert lib.ifx_attn_fwd_multi(small, 2, 12, 0.0, None) == -3 and b"item 1 (300 rows, 4000 keys) is a four-wave-kernel launch" in lib.ifx_last_error()

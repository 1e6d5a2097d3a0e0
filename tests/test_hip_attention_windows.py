"""Attention launches on MAGI's inputs against exact (fp64) attention: grouped-query heads, key windows that start inside a tile and
a page, page tables, two-segment views, strided q / out rows, split, partial and multi-range launches — on every schedule behind
`attn_variant`.  The data carries planted window-edge rows (attn_window_util.py): a kernel that reads kv head h % hk, or one key too
many or too few at either end of the window, misses the bound by two orders of magnitude (test_attn_window_oracle.py shows that on
the CPU).  Shapes are the smallest at which each path can go wrong; references are computed once per case and shared.
Run on the MI355X box: pytest -m gpu."""
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

from attn_window_util import BF, build_case, check, contiguous_slots, exact, figures, paged_slots, segment_slots

pytestmark = pytest.mark.gpu

K0 = 137                                   # window start: inside a 64-key tile, inside a page of every size used here
HEADS = [(3, 1), (6, 2), (24, 8), (4, 4)]
ROWS = [1, 33, 129, 257, 385]              # 129 / 257 / 385: one past the 128- / 256- / 384-row tiles of schedules 6 / 2,4,5,7 / 3
BASE = [1, 63, 64, 65, 69, 133, 197]       # 1, around one tile, 64 t + 5 for t = 1, 2, 3
DEEP = [64 * t + 5 for t in (4, 5, 6, 7, 13)]   # with BASE: every remainder of the four- and six-times unrolled loops (schedules 7, 6)


def _table(lengths, reps, salt):
    return [(ROWS[(i + 2 * j + salt) % 5],) + HEADS[(i + j) % 4] + (n,) for i, n in enumerate(lengths) for j in range(reps)]


# (rows, hq, hk, window length); the last one takes the multi-wave path under auto and the long-key four-wave kernel under variant 1
CASES = _table(BASE, 4, 0) + [(1030, 6, 2, 1100)]
CASES_DEEP = _table(DEEP, 2, 1)
for _t, _lengths in ((CASES, BASE + [1100]), (CASES + CASES_DEEP, BASE + DEEP)):
    assert {c[0] for c in _t} >= set(ROWS) and {c[1:3] for c in _t} == set(HEADS) and {c[3] for c in _t} >= set(_lengths)
SCHEDULE_CASES = [(v,) + c for v in range(8) for c in CASES + (CASES_DEEP if v in (6, 7) else [])]


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


@lru_cache(maxsize=None)
def _case(rows, hq, hk, n, prescaled=False):
    """One window [K0, K0 + n) of a cache of K0 + n + 9 keys with its references (computed once, never modified)."""
    k0, k1 = K0, K0 + n
    q, k, v = build_case(rows, hq, hk, k1 + 9, k0, k1, seed=rows + 7 * n + hq)
    q_call, scale = q, 0.0
    if prescaled:                          # q carries softmax_scale * log2(e), rounded to bf16 once; the call says scale = ln 2
        from inferix_amd import hip_ops
        q_scale, scale = hip_ops.attn_q_prescale(128)
        q_call = (q.float() * q_scale).to(BF)
    out64, lse64, ref_bf = exact(q, k, v, k0, k1, q_call if prescaled else None, scale)
    return SimpleNamespace(rows=rows, hq=hq, hk=hk, k0=k0, k1=k1, q=q_call, k=k, v=v, scale=scale, refs=(out64, lse64, ref_bf),
                           name=f"rows {rows} heads {hq}/{hk} keys [{k0}, {k1})" + (" prescaled" if prescaled else ""))


def _judge(section, what, out, lse, refs):
    """Print the figures (room inside the bounds), then apply the rule."""
    f = figures(out, lse, *refs)
    print(f"ATTNWIN|{section}|{what}|{f['err'] / f['err_bound']:.4f}|{f['rel'] / f['rel_bound']:.4f}|"
          f"{-1.0 if f['lse'] is None else f['lse']:.3e}")
    check(out, lse, *refs, what=what)


def _view(ops, c, kind, arg=None):
    """A physical view of the case's logical keys; unmapped slots hold NaN."""
    if kind == "contiguous":
        kc, vc = contiguous_slots(c.k, c.v)
        return ops.KvCacheView(kc.cuda(), vc.cuda())
    if kind == "page":
        kc, vc, table = paged_slots(c.k, c.v, arg)
        return ops.KvCacheView(kc.cuda(), vc.cuda(), table.cuda(), arg)
    split, delta = arg
    kc, vc = segment_slots(c.k, c.v, split, delta)
    return ops.KvCacheView(kc.cuda(), vc.cuda(), None, 1, split, delta)


def _attend(ops, c, view, splits=1):
    out, lse = ops.attention(c.q.cuda(), view, c.k1, scale=c.scale, kv_start=c.k0, return_lse=True, splits=splits)
    torch.cuda.synchronize()
    return out, lse


# ---- (a) every schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,rows,hq,hk,n", SCHEDULE_CASES)
def test_window_on_every_schedule(ops, variant, rows, hq, hk, n):
    c = _case(rows, hq, hk, n)
    with ops.option_scope("attn_variant", variant):
        out, lse = _attend(ops, c, _view(ops, c, "contiguous"))
    _judge("a", f"variant {variant} {c.name}", out, lse, c.refs)


# ---- (b) views ---------------------------------------------------------------------------------------------------------------------
N_VIEWS = 5 * 64 + 37                      # five key tiles and a ragged tail


@pytest.mark.parametrize("hq,hk", [(3, 1), (24, 8)])
@pytest.mark.parametrize("variant", range(8))
def test_window_through_page_tables_and_segments(ops, variant, hq, hk):
    """Pages of >= 3 rows and two-segment views translate wave-uniformly: the SAME schedule over the contiguous cache gives the same
    bits.  One- and two-row pages translate per lane (the multi-wave launches among them run schedule 2 whatever was asked)."""
    c = _case(257, hq, hk, N_VIEWS)
    k0, k1 = c.k0, c.k1
    views = [("page", ps) for ps in (64, 24, 7, 3, 2, 1)]
    views += [("segments", (split, 11)) for split in (k0 - 37, k0, k0 + 70, k1 - 1)]     # below, at, inside, at the last key
    with ops.option_scope("attn_variant", variant):
        plain, lse = _attend(ops, c, _view(ops, c, "contiguous"))
        _judge("b", f"variant {variant} contiguous {c.name}", plain, lse, c.refs)
        for kind, arg in views:
            out, lse = _attend(ops, c, _view(ops, c, kind, arg))
            _judge("b", f"variant {variant} {kind} {arg} {c.name}", out, lse, c.refs)
            if not (kind == "page" and arg < 3):
                assert torch.equal(out, plain), (variant, kind, arg, float((out.float() - plain.float()).abs().max()))


# ---- (c) exponent forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 3, 4, 5, 6, 7, 13])
@pytest.mark.parametrize("variant", [0, 6, 7])
def test_window_with_prescaled_q(ops, variant, t):
    for rows, hq, hk in ((257, 3, 1), (129, 6, 2)):
        c = _case(rows, hq, hk, 64 * t + 5, prescaled=True)
        with ops.option_scope("attn_variant", variant):
            for kind, arg in (("contiguous", None), ("segments", (c.k0 + 38, 11))):
                out, lse = _attend(ops, c, _view(ops, c, kind, arg))
                _judge("c", f"variant {variant} {kind} {c.name}", out, lse, c.refs)


# ---- (d) split and partial launches with grouped heads -----------------------------------------------------------------------------
N_SPLIT = 9 * 64 + 5                       # ten key tiles: 64 splits are clamped to ten chunks of one tile


@pytest.mark.parametrize("hq,hk", [(3, 1), (24, 8)])
@pytest.mark.parametrize("variant", range(8))
def test_window_split_and_partial_launches(ops, variant, hq, hk):
    c = _case(257, hq, hk, N_SPLIT)
    view = _view(ops, c, "contiguous")
    qg = c.q.cuda()
    with ops.option_scope("attn_variant", variant):
        for s in (2, 3, 64):
            out, lse = _attend(ops, c, view, splits=s)
            _judge("d", f"variant {variant} splits {s} {c.name}", out, lse, c.refs)
        # two partial launches over adjacent windows, the cut inside a tile, one workspace, one merge
        km = c.k0 + 4 * 64 + 29
        ws = ops.attention_workspace(qg, 5)
        u1 = ops.attention_partial(qg, view, km, c.k0, 2, ws, 0, 5)
        u2 = ops.attention_partial(qg, view, c.k1, km, 3, ws, u1, 5)
        assert (u1, u2) == (2, 3)
        out = torch.full_like(qg, float("nan"))
        lse = torch.full((hq, c.rows), float("nan"), dtype=torch.float32, device="cuda")
        ops.attention_merge(ws, 5, u1 + u2, out, lse)
        torch.cuda.synchronize()
    _judge("d", f"variant {variant} partial [{c.k0}, {km}) + [{km}, {c.k1}) {c.name}", out, lse, c.refs)


# ---- (e) strided rows --------------------------------------------------------------------------------------------------------------
def _wide_q(q2d, hq):
    """q as the column block at offset 64 of a [rows, 2 * hq * 128 + 64] matrix of NaN."""
    wide = torch.full((q2d.shape[0], 2 * hq * 128 + 64), float("nan"), dtype=BF)
    wide[:, 64:64 + hq * 128] = q2d
    return wide.cuda()


@pytest.mark.parametrize("hq,hk", [(3, 1), (24, 8)])
@pytest.mark.parametrize("variant", [0, 1, 6, 7])
def test_window_with_strided_rows(ops, variant, hq, hk):
    c = _case(257, hq, hk, N_VIEWS)
    view = _view(ops, c, "segments", (c.k0 + 70, 11))
    d = hq * 128
    wq = _wide_q(c.q.view(c.rows, d), hq)
    with ops.option_scope("attn_variant", variant):
        for splits in (None, 1, 3):        # 3: the partials are merged into the strided rows
            wo = torch.full((c.rows, 2 * d), 7.0, dtype=BF, device="cuda")
            ops.attention_ld(wq[:, 64:64 + d], view, c.k1, wo[:, d:], hq, kv_start=c.k0, splits=splits)
            torch.cuda.synchronize()
            assert bool((wo[:, :d] == 7.0).all()), (variant, splits, "columns beside the output block were written")
            _judge("e", f"variant {variant} splits {splits} {c.name}", wo[:, d:].reshape(c.rows, hq, 128), None, c.refs)


# ---- (f) multi-range launches ------------------------------------------------------------------------------------------------------
# ranges as (query rows, first key, keys) in the order they are given to the launch; `place`: the order in which their query rows
# lie in the matrix (gaps of 5 rows between them, 3 in front).
# No window holds another range's decoy (_ranges_case asserts it), so windows overlap through the one-row ranges, which plant none.
# Why: a decoy inside a window is a legitimate key with |v| = 64, and rows that put most of their weight on it come out at ~56, where a
# bf16 ulp is 0.25.  The yardstick (SDPA on the CPU) keeps P in fp32, so its whole error there is the final rounding (<= 0.125); a kernel
# that rounds P to bf16, as these and FlashAttention do, adds |v| * P * 2^-9 ~ 0.11 on top whenever the dominant P is not exactly 1
# (the lazy reference maximum) — twice the yardstick's error by construction, not by defect: the rule's factor 2 presumes |v| ~ 1.
# (Measured on a layout with such a decoy: max error 0.2984 against a bound of 0.2981 under the automatic schedule; a CPU evaluation with P
# rounded to bf16 against the first tile's maximum gives the same 0.2984 to ten digits.)
RANGE_CAP = 1100
LAYOUTS = {
    "n1": ([(257, 137, 357)], [0]),
    # ascending key-window length: the host's longest-first order is the reverse
    "n3": ([(257, 137, 69), (129, 300, 197), (1, 520, 325)], [1, 2, 0]),
    # two windows of 197 keys (a tie of the sort); [300, 497), [402, 727) and the one-key window [500, 501) overlap each other and [211, 792)
    "n8": ([(129, 137, 69), (1, 300, 197), (257, 211, 581), (1, 500, 1), (257, 1003, 66), (129, 800, 197), (1, 402, 325), (129, 5, 125)],
           [5, 2, 7, 0, 4, 1, 6, 3]),
}


@lru_cache(maxsize=None)
def _ranges_case(layout, hq, hk):
    ranges, place = LAYOUTS[layout]
    g = torch.Generator().manual_seed(900 + hq)
    k = torch.randn(RANGE_CAP, hk, 128, generator=g).to(BF)
    v = torch.randn(RANGE_CAP, hk, 128, generator=g).to(BF)
    qs, planted = [], set()
    decoys = [{ks - 1, ks + kl} if ql >= 4 else set() for ql, ks, kl in ranges]
    assert not any(ks <= key < ks + kl for i, (_, ks, kl) in enumerate(ranges) for j, dj in enumerate(decoys) if i != j for key in dj), \
        "a window must not hold another range's decoy (see LAYOUTS)"
    for i, (ql, ks, kl) in enumerate(ranges):
        # one build_case per range plants that range's edge rows; they go into the shared cache
        q_r, k_r, v_r = build_case(ql, hq, hk, RANGE_CAP, ks, ks + kl, seed=500 + 10 * i + hq)
        edge = {ks, ks + kl - 1} | ({ks - 1, ks + kl} if ql >= 4 else set())
        assert not (edge & planted), "the ranges' edge keys must be distinct"
        planted |= edge
        for key in edge:
            k[key], v[key] = k_r[key], v_r[key]
        qs.append(q_r)
    q_ranges, row = [None] * len(ranges), 3
    for i in place:
        q_ranges[i] = (row, row + ranges[i][0])
        row += ranges[i][0] + 5
    k_ranges = [(ks, ks + kl) for _, ks, kl in ranges]
    refs = [exact(q_r, k, v, ks, ke) for q_r, (ks, ke) in zip(qs, k_ranges)]
    q2d = torch.full((row, hq * 128), float("nan"), dtype=BF)         # rows of no range are never read
    for q_r, (a, b) in zip(qs, q_ranges):
        q2d[a:b] = q_r.view(b - a, -1)
    assert row <= 1030
    return SimpleNamespace(rows=row, hq=hq, hk=hk, k=k, v=v, q2d=q2d, q_ranges=q_ranges, k_ranges=k_ranges, refs=refs)


@pytest.mark.parametrize("view_kind,view_arg", [("contiguous", None), ("segments", (450, 11)), ("page", 24), ("page", 2)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("hq,hk", [(3, 1), (24, 8)])
def test_multi_range_launch(ops, hq, hk, layout, view_kind, view_arg):
    """One launch over several (query range, key window) pairs, each range judged against exact attention over ITS window.  A range
    launch asked for a schedule that is not software-pipelined runs schedule 7: variant 2 gives the bits of variant 7.  Over one- and
    two-row pages (per-lane translation) every range launch runs the plain two-group schedule."""
    c = _ranges_case(layout, hq, hk)
    view = _view(ops, c, view_kind, view_arg)
    d = hq * 128
    wq = _wide_q(c.q2d, hq)
    inside = torch.zeros(c.rows, dtype=torch.bool)
    for a, b in c.q_ranges:
        inside[a:b] = True
    outs = {}
    for variant in (0, 5, 6, 7, 2):
        wo = torch.full((c.rows, 2 * d), 3.0, dtype=BF, device="cuda")
        with ops.option_scope("attn_variant", variant):
            ops.attention_ranges(wq[:, 64:64 + d], view, c.q_ranges, c.k_ranges, wo[:, d:], hq)
        torch.cuda.synchronize()
        wo = wo.cpu()
        assert bool((wo[:, :d] == 3.0).all()) and bool((wo[~inside] == 3.0).all()), (variant, "rows or columns of no range were written")
        for i, ((a, b), refs) in enumerate(zip(c.q_ranges, c.refs)):
            _judge("f", f"variant {variant} {layout} {view_kind} {view_arg} heads {hq}/{hk} range {i} rows [{a}, {b}) keys {c.k_ranges[i]}",
                   wo[a:b, d:].reshape(b - a, hq, 128), None, refs)
        outs[variant] = wo
    assert torch.equal(outs[2], outs[7])

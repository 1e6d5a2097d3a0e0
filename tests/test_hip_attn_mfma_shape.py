"""GPU: the two matrix-instruction forms of the four-times-unrolled constant-slot attention loop (schedule 7) — option attn_mfma
1 = v_mfma_f32_32x32x16_bf16, 2 = v_mfma_f32_16x16x32_bf16 — on identical inputs, each against fp64 attention of the same bf16 inputs
by the rule of `_attn_case` (test_hip_kernels.py), and the new form against the old one: rel-L2 of form 2 from fp64 at most
1.25 x that of form 1 + 1e-6 (bit identity is not asked for: the key order inside a k-step and the row-sum order differ).

Shapes are the smallest at which each path can go wrong; a case's inputs and references are built once and shared by both forms."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import wan_oracle as O
from attn_window_util import build_case, check, contiguous_slots, exact
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = 128
FORMS = (1, 2)
TILES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13)      # every remainder of the four-times-unrolled loop, twice and more


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def _options_back(ops):
    yield
    ops.set_option("attn_mfma", 0)
    ops.set_option("attn_variant", 0)
    ops.set_option("attn_debug_counters", 0)


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g).to(BF)


@lru_cache(maxsize=None)
def _case(rows, heads, kv_len, cap, page, prescaled):
    """Inputs of `_attn_case` (same generator, same order) with the fp64 reference and the yardstick; never modified."""
    from inferix_amd import hip_ops
    g = torch.Generator().manual_seed(rows + kv_len)
    q = _rnd(g, rows, heads, HD)
    q_call, scale = q, 0.0
    if prescaled:
        q_scale, scale = hip_ops.attn_q_prescale(HD)
        q_call = (q.float() * q_scale).to(BF)
    k, v = _rnd(g, kv_len, heads, HD), _rnd(g, kv_len, heads, HD)
    if page is None:
        kc = torch.full((cap, heads, HD), float("nan"), dtype=BF)     # garbage beyond kv_len must not leak
        vc = torch.full((cap, heads, HD), float("nan"), dtype=BF)
        kc[:kv_len], vc[:kv_len] = k, v
        table = None
    else:
        npg = (cap + page - 1) // page
        perm = torch.randperm(npg, generator=g)
        kc, vc = torch.zeros(npg * page, heads, HD, dtype=BF), torch.zeros(npg * page, heads, HD, dtype=BF)
        t = torch.arange(kv_len)
        slot = perm[t // page] * page + t % page
        kc[slot], vc[slot] = k, v
        table = perm.to(torch.int32)
    q64 = q_call.double() * (scale * math.sqrt(HD)) if prescaled else q
    ref64, lse64 = O.attention_with_lse(q64[None], k[None], v[None])
    ref_bf = O.attention(q[None], k[None], v[None])
    return SimpleNamespace(q=q_call, kc=kc, vc=vc, table=table, page=page, kv_len=kv_len, scale=scale, ref64=ref64[0], lse64=lse64[0],
                           ref_bf=ref_bf[0], name=f"{rows} x {heads} x {kv_len}" + (f" page {page}" if page else "") + (" prescaled" if prescaled else ""))


def _launch(ops, c, form, splits=1):
    view = ops.KvCacheView(c.kc.cuda(), c.vc.cuda()) if c.table is None else ops.KvCacheView(c.kc.cuda(), c.vc.cuda(), c.table.cuda(), c.page)
    ops.set_option("attn_variant", 7)
    ops.set_option("attn_mfma", form)
    out, lse = ops.attention(c.q.cuda(), view, c.kv_len, scale=c.scale, return_lse=True, splits=splits)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu()


def _new_against_old(rel, what):
    print(f"ATTNMFMA|{what}|rel-L2 form 1 {rel[1]:.4e}|form 2 {rel[2]:.4e}|ratio {rel[2] / max(rel[1], 1e-30):.4f}")
    assert rel[2] <= 1.25 * rel[1] + 1e-6, (what, rel)


def _both_forms(ops, c, splits=1):
    """The checks of `_attn_case` on each form, then form 2 against form 1."""
    rel = {}
    for form in FORMS:
        out, lse = _launch(ops, c, form, splits)
        err_gpu = (out.double() - c.ref64).abs().max().item()
        err_ref = (c.ref_bf.double() - c.ref64).abs().max().item()
        rel[form] = rel_l2(out, c.ref64)
        assert math.isfinite(err_gpu), (form, c.name)
        assert err_gpu <= 2 * err_ref + 4e-3, (form, c.name, err_gpu, err_ref)
        assert rel[form] <= max(1.5 * rel_l2(c.ref_bf, c.ref64), 3e-3), (form, c.name, rel[form])
        assert (lse.double() - c.lse64).abs().max().item() < 2e-3, (form, c.name)
    _new_against_old(rel, c.name)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("tiles", TILES)
def test_every_loop_remainder(ops, tiles, prescaled):
    """Keys 64 t - 9 (contiguous, ragged last tile) and 64 t (pages of 64): 260 rows x 2 heads and 140 rows x 3 heads."""
    _both_forms(ops, _case(260, 2, 64 * tiles - 9, 64 * tiles, None, prescaled))
    _both_forms(ops, _case(140, 3, 64 * tiles, 64 * tiles + 64, 64, prescaled))


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("rows,kv_len", [(70, 40), (8, 200), (17, 200), (256 + 72, 200)])
def test_ragged_queries(ops, rows, kv_len, prescaled):
    """The last wave partly or wholly past the end of the rows, in both 16-query blocks of a lane: 70 rows (wave 2 holds 6 rows of its
    first block, none of its second), 8 and 17 rows (half a block; one block and one row), 256 + 72 (a second workgroup with 72 rows)."""
    _both_forms(ops, _case(rows, 2, kv_len, kv_len + 24, None, prescaled))


@lru_cache(maxsize=None)
def _planted():
    """The planted-key case of test_attention_prescaled_q_exponent_fast_path: 300 x 2 x 900, three keys that dominate late."""
    from inferix_amd import hip_ops
    g = torch.Generator().manual_seed(3)
    rows, heads, kv_len = 300, 2, 900
    q, k, v = _rnd(g, rows, heads, HD), _rnd(g, kv_len, heads, HD), _rnd(g, kv_len, heads, HD)
    k[500] = (q[5] * 4).to(BF)
    k[10] = (q[40] * 6).to(BF)
    k[700] = (q[290] * 5).to(BF)
    q_scale, scale = hip_ops.attn_q_prescale(HD)
    qs = (q.float() * q_scale).to(BF)
    ref64, _ = O.attention_with_lse((qs.double() * (scale * math.sqrt(HD)))[None], k[None], v[None])
    return SimpleNamespace(q=qs, k=k, v=v, kv_len=kv_len, scale=scale, ref64=ref64[0])


def test_redo_path_runs_under_the_new_form(ops):
    """A tile outgrows the lazy reference maximum: redo against the true maximum, O and l rescaled, the next tile's scores (already
    computed as S - m) corrected.  The rescale counter proves that the branch ran under form 2."""
    c = _planted()
    rel = {}
    for form in FORMS:
        ops.set_option("attn_variant", 7)
        ops.set_option("attn_mfma", form)
        ops.set_option("attn_debug_counters", 1)          # allocates and zeroes the counter
        out = ops.attention(c.q.cuda(), ops.KvCacheView(c.k.cuda(), c.v.cuda()), c.kv_len, scale=c.scale, splits=1)
        torch.cuda.synchronize()
        taken = ops.get_option("attn_rescale_count")
        ops.set_option("attn_debug_counters", 0)
        print(f"ATTNMFMA|planted keys|form {form}|rescale branches {taken}")
        assert taken > 0, f"form {form}: the rescale branch did not run"
        out = out.cpu()
        assert (out.double() - c.ref64).abs().max().item() < 3e-2
        rel[form] = rel_l2(out, c.ref64)
        assert rel[form] < 5e-3
    _new_against_old(rel, "planted keys 300 x 2 x 900")


def _window_both_forms(ops, run, refs_list, what):
    """`run(form)` -> list of (out, lse or None), one per entry of `refs_list`: the window rule on each form, then new against old."""
    num, den = {}, {}
    for form in FORMS:
        ops.set_option("attn_variant", 7)
        ops.set_option("attn_mfma", form)
        outs = run(form)
        torch.cuda.synchronize()
        num[form] = den[form] = 0.0
        for i, ((out, lse), refs) in enumerate(zip(outs, refs_list)):
            f = check(out, lse, *refs, what=f"{what} form {form} part {i}")
            num[form] += float(((out.detach().cpu().double() - refs[0]) ** 2).sum())
            den[form] += float((refs[0] ** 2).sum())
    _new_against_old({f: math.sqrt(num[f] / den[f]) for f in FORMS}, what)


@lru_cache(maxsize=None)
def _gqa_case():
    k0, k1 = 137, 137 + 133                  # the window starts inside a tile: three key tiles, ragged
    q, k, v = build_case(257, 6, 2, k1 + 9, k0, k1, seed=257 + 7 * 133 + 6)
    return SimpleNamespace(q=q, k=k, v=v, k0=k0, k1=k1, refs=exact(q, k, v, k0, k1))


def test_grouped_query_heads(ops):
    """6 query heads on 2 kv heads, 257 rows (one past a 256-row tile), a key window with planted edge rows and decoys."""
    c = _gqa_case()
    kc, vc = contiguous_slots(c.k, c.v)

    def run(form):
        out, lse = ops.attention(c.q.cuda(), ops.KvCacheView(kc.cuda(), vc.cuda()), c.k1, kv_start=c.k0, return_lse=True, splits=1)
        return [(out, lse)]
    _window_both_forms(ops, run, [c.refs], "GQA 257 x 6/2 keys [137, 270)")


@lru_cache(maxsize=None)
def _ranges_case():
    hq, hk, cap = 3, 1, 520
    ranges = [(257, 137, 69), (129, 300, 197)]            # (query rows, first key, keys); shorter window first: the host sorts
    g = torch.Generator().manual_seed(903)
    k, v = torch.randn(cap, hk, HD, generator=g).to(BF), torch.randn(cap, hk, HD, generator=g).to(BF)
    qs = []
    for i, (ql, ks, kl) in enumerate(ranges):
        q_r, k_r, v_r = build_case(ql, hq, hk, cap, ks, ks + kl, seed=500 + 10 * i + hq)
        for key in (ks - 1, ks, ks + kl - 1, ks + kl):     # this range's edge rows and decoys go into the shared cache
            k[key], v[key] = k_r[key], v_r[key]
        qs.append(q_r)
    q_ranges = [(134 + 5, 134 + 5 + 257), (3, 3 + 129)]   # the second range's rows lie first; gaps of rows that belong to no range
    rows = q_ranges[0][1] + 5
    k_ranges = [(ks, ks + kl) for _, ks, kl in ranges]
    refs = [exact(q_r, k, v, ks, ke) for q_r, (ks, ke) in zip(qs, k_ranges)]
    q2d = torch.full((rows, hq * HD), float("nan"), dtype=BF)
    for q_r, (a, b) in zip(qs, q_ranges):
        q2d[a:b] = q_r.view(b - a, -1)
    return SimpleNamespace(rows=rows, hq=hq, k=k, v=v, q2d=q2d, q_ranges=q_ranges, k_ranges=k_ranges, refs=refs)


def test_multi_range_launch(ops):
    """Two (query range, key window) pairs in one launch, each judged over its own window; rows of no range stay untouched."""
    c = _ranges_case()
    kc, vc = contiguous_slots(c.k, c.v)
    d = c.hq * HD
    inside = torch.zeros(c.rows, dtype=torch.bool)
    for a, b in c.q_ranges:
        inside[a:b] = True

    def run(form):
        wo = torch.full((c.rows, d), 3.0, dtype=BF, device="cuda")
        ops.attention_ranges(c.q2d.cuda(), ops.KvCacheView(kc.cuda(), vc.cuda()), c.q_ranges, c.k_ranges, wo, c.hq)
        torch.cuda.synchronize()
        wo = wo.cpu()
        assert bool((wo[~inside] == 3.0).all()), (form, "rows of no range were written")
        return [(wo[a:b].reshape(b - a, c.hq, HD), None) for a, b in c.q_ranges]
    _window_both_forms(ops, run, c.refs, "two ranges 257 x [137, 206) + 129 x [300, 497), heads 3/1")

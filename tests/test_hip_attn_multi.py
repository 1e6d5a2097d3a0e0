"""ifx_attn_fwd_multi on the GPU: every item of a multi launch is BIT-IDENTICAL to its own unsplit single launch in the same loop form
(forced attn_variant 6 / 7, attn_mfma 1 / 2, with and without the exponent form), whatever its neighbours in the launch are; nothing
outside an item's output block is written; what the entry point does not build is refused by return code and message."""
import pytest
import torch

import attn_multi_util as U

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = 128
PAD, SIDE = 3, 64               # sentinel rows above / below every out block, sentinel columns on both sides
SENTINEL = 1024.0


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


@pytest.fixture(autouse=True)
def _options_back(ops):
    yield
    ops.set_option("attn_mfma", 0)
    ops.set_option("attn_variant", 0)


# (q rows, kv_start, kv_len, page size or None, table rotated).  Rows {300, 256, 37, 129}: ragged last query tiles of both tile sizes
# (128, 256), an exact tile, less than one wave.  Keys {465, 1, 63, 64, 833}: 8 and 14 tiles (the four- and six-times unrolled loops
# wrap their rings), one key, one short of a tile, an exact tile, ragged last tiles.  Listed SHORTEST first: the launch order permutes them.
MAIN = [(37, 0, 1, None, 0), (129, 0, 63, None, 0), (256, 40, 104, None, 0), (300, 0, 465, None, 0), (129, 0, 833, None, 0)]
ONE = [(300, 0, 465, None, 0)]
TWO = [(300, 0, 833, None, 0), (256, 0, 465, None, 0)]          # two caches, query rows neighbours in ONE buffer
EIGHT = [(r, 0, k, None, 0) for r, k in zip((37, 129, 256, 300, 37, 129, 256, 300), (1, 63, 64, 465, 833, 465, 833, 64))]
PAGED = [(37, 0, 63, 8, 0), (256, 0, 64, 64, 0), (129, 5, 465, 8, 1), (300, 0, 833, 64, 1)]       # fresh tables beside rotated ones
SETS = {"main": MAIN, "one": ONE, "two": TWO, "eight": EIGHT, "paged": PAGED}
_WORLD = {}


def _world(ops, name, hq, hk):
    """The inputs of item set `name` on the device, made once and never modified: per item (q view, KvCacheView)."""
    key = (name, hq, hk)
    if key in _WORLD:
        return _WORLD[key]
    g = torch.Generator().manual_seed(len(name) + hq)
    W = hq * HD + 2 * SIDE
    rows = sum(it[0] for it in SETS[name])
    qbuf = torch.randn(rows, W, generator=g).to(BF).cuda()          # one buffer: consecutive items' rows are neighbours
    items, r0 = [], 0
    for rws, k0, k1, ps, rot in SETS[name]:
        cap = k1 + 5
        k, v = torch.randn(cap, hk, HD, generator=g).to(BF), torch.randn(cap, hk, HD, generator=g).to(BF)
        k[k1:], v[k1:] = float("nan"), float("nan")                  # keys behind the range must not leak
        if k0:
            k[:k0], v[:k0] = float("nan"), float("nan")
        if ps is None:
            view = ops.KvCacheView(k.cuda(), v.cuda())
        else:
            npg = (cap + ps - 1) // ps + 2
            perm = torch.randperm(npg, generator=g) if rot else torch.arange(npg)
            kc, vc = torch.full((npg * ps, hk, HD), float("nan"), dtype=BF), torch.full((npg * ps, hk, HD), float("nan"), dtype=BF)
            t = torch.arange(cap)
            slot = perm[t // ps] * ps + t % ps
            kc[slot], vc[slot] = k, v
            view = ops.KvCacheView(kc.cuda(), vc.cuda(), perm.to(torch.int32).cuda(), ps)
        items.append((qbuf[r0:r0 + rws, SIDE:SIDE + hq * HD], view, k0, k1))
        r0 += rws
    _WORLD[key] = (items, W)
    return _WORLD[key]


def _run(ops, name, hq, hk, variant, mfma, pre):
    items, W = _world(ops, name, hq, hk)
    q_scale, scale = ops.attn_q_prescale(HD) if pre else (1.0, 0.0)
    ops.set_option("attn_variant", variant)
    ops.set_option("attn_mfma", mfma)
    rows = sum(q.shape[0] for q, *_ in items)
    obuf = torch.full((rows + PAD * (len(items) + 1), W), SENTINEL, dtype=BF, device="cuda")
    mask = torch.ones_like(obuf, dtype=torch.bool)                   # True: must still hold the sentinel afterwards
    call, refs, r0 = [], [], PAD
    for q, view, k0, k1 in items:
        qc = (q.float() * q_scale).to(BF) if pre else q
        # strided q: the scaled copy sits in a wider buffer again
        qw = torch.zeros(q.shape[0], W, dtype=BF, device="cuda")
        qw[:, SIDE:SIDE + hq * HD] = qc
        out = obuf[r0:r0 + q.shape[0], SIDE:SIDE + hq * HD]
        mask[r0:r0 + q.shape[0], SIDE:SIDE + hq * HD] = False
        call.append((qw[:, SIDE:SIDE + hq * HD], view, k1, out, k0))
        refs.append(ops.attention(qc.contiguous().view(-1, hq, HD), view, k1, scale=scale, kv_start=k0, splits=1))
        r0 += q.shape[0] + (0 if name == "two" else PAD)             # "two": the out blocks are neighbours as well
    ops.attention_multi(call, hq, scale=scale)
    torch.cuda.synchronize()
    for i, ((_, _, _, out, _), ref) in enumerate(zip(call, refs)):
        assert torch.isfinite(ref.float()).all(), (name, i)
        assert torch.equal(out.reshape(-1, hq, HD), ref), \
            f"{name} item {i} {SETS[name][i]}: variant {variant} mfma {mfma} pre {pre}: differs from its single launch " \
            f"(max abs {(out.reshape(-1, hq, HD).float() - ref.float()).abs().max().item():.3e})"
    assert bool((obuf[mask] == SENTINEL).all()), f"{name}: variant {variant} mfma {mfma} pre {pre}: written outside an item's out block"


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("mfma", [1, 2])
@pytest.mark.parametrize("variant", [6, 7])
@pytest.mark.parametrize("name", ["main", "one", "two", "eight", "paged"])
def test_items_equal_their_single_launches(ops, name, variant, mfma, pre):
    _run(ops, name, 12, 12, variant, mfma, pre)


@pytest.mark.parametrize("variant,mfma", [(6, 1), (7, 1), (7, 2)])
def test_grouped_query_heads(ops, variant, mfma):
    _run(ops, "main", 4, 2, variant, mfma, True)
    _run(ops, "paged", 4, 2, variant, mfma, False)


def test_multi_launch_is_taken(ops, monkeypatch):
    """The comparisons above are of the multi launch: ops.attention_multi does not reach the per-item path for these sets."""
    def no_fallback(*a, **kw):
        raise AssertionError("attention_multi fell back to per-item launches")
    ops.set_option("attn_variant", 7)
    items, W = _world(ops, "main", 12, 12)
    outs = [torch.empty(q.shape[0], 12 * HD, dtype=BF, device="cuda") for q, *_ in items]
    monkeypatch.setattr(ops, "attention_ld", no_fallback)
    ops.attention_multi([(q, view, k1, o, k0) for (q, view, k0, k1), o in zip(items, outs)], 12)
    torch.cuda.synchronize()


def test_wrapper_groups_and_falls_back(ops):
    """Ten items of both view kinds plus a two-segment view: the wrapper launches the groups the entry point takes and the rest one by
    one; under the automatic choice these small items all go one by one.  Every result is the single launch's."""
    cont, _ = _world(ops, "eight", 12, 12)
    paged, _ = _world(ops, "paged", 12, 12)
    q, view, k0, k1 = cont[3]
    seg = ops.KvCacheView(torch.cat([view.k[:100], view.k[:8], view.k[100:]]).contiguous(),
                          torch.cat([view.v[:100], view.v[:8], view.v[100:]]).contiguous(), seg_split=100, seg_delta=8)
    everything = list(cont) + list(paged[:2]) + [(q, seg, k0, k1)]
    for variant in (7, 0):
        ops.set_option("attn_variant", variant)
        outs = [torch.empty(q.shape[0], 12 * HD, dtype=BF, device="cuda") for q, *_ in everything]
        ops.attention_multi([(q, v, k1, o, k0) for (q, v, k0, k1), o in zip(everything, outs)], 12)
        for (q, v, k0, k1), o in zip(everything, outs):
            ref = ops.attention(q.contiguous().view(-1, 12, HD), v, k1, kv_start=k0, splits=1 if variant else None)
            assert torch.equal(o.view(-1, 12, HD), ref), (variant, q.shape, k0, k1)


def test_refusals(ops):
    from inferix_amd import _hip
    U.check_refusals(_hip, lambda v: ops.set_option("attn_variant", v))

"""The grouped split-key launch of the 8-bit ring cache (ifx_attn_fwd_kv8_grouped_split) on the GPU: against fp64 attention under the
rule of test_hip_attn_kv8_ring.py, its exactness and reuse properties, and the tiny ring rollout with the model asking the plan."""
import pytest
import torch

from test_hip_attn_kv8 import HD, _attn_reference
from test_hip_attn_kv8_ring import _case, ops  # noqa: F401 (ops: fixture)
from test_hip_kv8_ring_model import _emulated_oracle_rollout, _rollout
from util import rel_l2

pytestmark = pytest.mark.gpu
#        (rows hq hk G kv_len), splits, kind
CASES = [((33, 2, 1, 24, 72), 3, ""),                 # a group smaller than a tile: one group per chunk; GQA
         ((65, 2, 2, 100, 300), 2, ""),               # a partial tile in every group; the chunk boundary falls inside group 1
         ((300, 4, 2, 128, 448), 3, ""),              # two row tiles, GQA, last group partial; 7 tiles dealt 3 / 2 / 2
         ((33, 2, 2, 64, 1024), 16, ""),              # sixteen one-tile chunks: every chunk has a scale of its own
         ((33, 2, 2, 64, 1025), 16, ""),              # ... and a 17th tile of one key
         ((33, 4, 2, 100, 300), 8, ""),               # chunks clamp to 6
         ((300, 2, 2, 1560, 4680), 4, ""),            # the real frame: 75 tiles, boundaries inside groups
         ((300, 4, 2, 128, 448), 2, "strided"),       # q / out windows of wider buffers
         ((33, 2, 2, 100, 325), 5, "rising")]         # scores rise ~3 per 64 keys: chunk maxima apart, merge weights towards 0


def _launch(ops, shape, splits, kind="", poison=True, equal=False):
    # "rising": the flat test's rising case (one scale per head) behind a ring view: NaN bytes up to whole groups, equal table rows
    rows, hq, hk, G, kv_len = shape
    if kind == "rising":
        q8, k8, v8, v_scale, out64, lse64, emu64 = _attn_reference((rows, hq, hk, 0, kv_len, False, True))
        pad = torch.full((-(-k8.shape[0] // G) * G - k8.shape[0], hk, HD), 0x7F, dtype=torch.uint8)
        k8, v8, scale = torch.cat([k8, pad]), torch.cat([v8, pad]), v_scale.repeat(-(-k8.shape[0] // G), 1)
    else:
        q8, k8, v8, scale, out64, lse64, emu64 = _case(*shape, equal=equal)
    view = ops.Kv8RingView(k8.cuda(), v8.cuda(), scale.cuda(), G)
    qg, og, obuf = q8.cuda(), None, None
    if kind == "strided":
        qbuf = torch.full((rows, hq * HD + 48), 0x7F, dtype=torch.uint8, device="cuda")
        obuf = torch.full((rows, hq * HD + 24), 7.0, dtype=torch.bfloat16, device="cuda")
        qg, og = qbuf[:, 16:16 + hq * HD].view(rows, hq, HD), obuf[:, 8:8 + hq * HD].view(rows, hq, HD)
        qg.copy_(q8)
    if poison:          # the WHOLE workspace, arrival counters included: nothing it held may matter
        need = ops.attention_kv8_grouped_split_plan(rows, hq, G, kv_len, splits)["workspace_bytes"]
        ops._kv8_split_workspace(qg.device, need).view(torch.uint8).fill_(0xFF)
    out, lse = ops.attention_kv8_grouped(qg, view, kv_len, out=og, return_lse=True, splits=splits)
    return out, lse, obuf, out64, lse64, emu64


@pytest.mark.parametrize("shape,splits,kind", CASES, ids=lambda c: "-".join(str(x) for x in c) if isinstance(c, tuple) else f"{c}")
def test_grouped_split_against_fp64(ops, shape, splits, kind):
    rows, hq, _, G, kv_len = shape
    plan = ops.attention_kv8_grouped_split_plan(rows, hq, G, kv_len, splits)
    assert plan["chunks"] == min(splits, plan["key_tiles"]) > 1 and rows * hq >= 64      # (the rule pools at least 64 softmax rows)
    out, lse, obuf, out64, lse64, emu64 = _launch(ops, shape, splits, kind)
    if obuf is not None:
        assert bool((obuf[:, :8] == 7.0).all()) and bool((obuf[:, 8 + hq * HD:] == 7.0).all()), "columns outside the output window were written"
    rel, rel_emu = rel_l2(out.cpu(), out64), rel_l2(emu64, out64)
    lse_err = (lse.cpu().double() - lse64).abs().max().item()
    print(f"attention_kv8_grouped split {shape} x{splits} {kind}: rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}, lse err {lse_err:.2e}")
    assert rel <= 1.25 * rel_emu + 1e-3 and lse_err <= 2e-3          # (NaN compares false)


def test_exactness_and_reuse(ops):
    # a split request that clamps to one chunk (one tile of 24 keys) is the unsplit grouped launch, bit for bit
    assert ops.attention_kv8_grouped_split_plan(65, 2, 24, 24, 4)["workspace_bytes"] == 0
    (a, la), (b, lb) = (_launch(ops, (65, 2, 1, 24, 24), n, poison=False)[:2] for n in (4, 1))
    assert torch.equal(a, b) and torch.equal(la, lb)
    # equal scales and whole tiles: n chunks are the flat split launch's n chunks on the same bytes
    shape = (300, 4, 2, 128, 448)
    q8, k8, v8, scale = _case(*shape, equal=True)[:4]
    a, la = _launch(ops, shape, 3, equal=True)[:2]
    b, lb = ops.attention_kv8(q8.cuda(), ops.Kv8CacheView(k8.cuda(), v8.cuda(), scale[0].cuda()), 448, return_lse=True, splits=3)
    assert torch.equal(a, b) and torch.equal(la, lb)
    # the same split launch twice, the second on the workspace the first left behind: the merge order is the chunk order
    a, la = _launch(ops, shape, 3)[:2]
    b, lb = _launch(ops, shape, 3, poison=False)[:2]
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_rolling_rollout_ring_split(ops, monkeypatch):
    """With chunks of one tile allowed the tiny ring rollout's forwards split (72 rows x 2 heads, up to 144 keys in groups of 24); trace
    and distance rule are test_rolling_rollout_kv8_ring's.  `kv8_ring_split=False` under the same option is the parent run, bit for bit."""
    from fixture_io import golden
    fx = golden("rollout_tiny_local.npz")
    parent = _rollout(fx, kv_cache_dtype="fp8_e4m3_ring")[0]
    with ops.option_scope("attn_kv8_grouped_split_min_tiles", 1):
        out8, trace8 = _rollout(fx, kv_cache_dtype="fp8_e4m3_ring", kv8_ring_split=True)
        off = _rollout(fx, kv_cache_dtype="fp8_e4m3_ring", kv8_ring_split=False)[0]
        chunks = ops.attention_kv8_grouped_split_plan(3 * 24, 2, 24, max(t[2] for t in trace8))["chunks"]
    assert chunks > 1, chunks
    assert trace8 == [tuple(r) for r in fx["trace"].tolist()]
    assert torch.equal(off, parent)
    assert not torch.equal(out8, parent), "the model did not take the split launch"
    d8, d_emu = rel_l2(out8, fx["out"]), rel_l2(_emulated_oracle_rollout(fx, monkeypatch), fx["out"])
    print(f"rollout_tiny_local, split grouped attention vs the oracle rollout: {d8:.3e}; oracle with the emulated format {d_emu:.3e}")
    assert d8 <= 1.5 * d_emu

"""The split-key launch of the 8-bit self-attention (ifx_attn_fwd_kv8_split) on the GPU: against fp64 attention over the dequantised
bytes under the rule of test_hip_attn_kv8.py, its exactness and reuse properties, and the tiny rollout with the model asking the plan."""
import pytest
import torch

from test_hip_attn_kv8 import HD, Q_SCALE, _attn_reference, _emulated_oracle_rollout, _rollout, e4m3  # noqa: F401  (e4m3, Q_SCALE: the emulation's)
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


#        (rows hq hk kv_start keys strided rising), splits
CASES = [((33, 2, 2, 0, 64 * 5 + 5, False, False), 3),       # row-tile tail; ragged last chunk
         ((300, 4, 2, 0, 64 * 5 + 5, False, False), 3),      # two row tiles, grouped-query heads
         ((33, 2, 2, 70, 200, False, False), 2),             # non-zero key start
         ((33, 4, 2, 0, 64 * 3, False, False), 8),           # chunks clamp to 3
         ((33, 2, 2, 0, 64 * 16, False, False), 16),         # the chunk maximum, one tile each
         ((300, 2, 2, 0, 64 * 16 + 1, False, False), 16),    # ... and a 17th tile of one key
         ((33, 2, 2, 0, 64 * 5 + 5, False, True), 5),        # rising scores: chunk maxima ~3 apart per tile, merge weights towards 0
         ((300, 4, 2, 0, 200, True, False), 2)]              # strided q / out


def _launch(ops, case, splits, poison=True):
    rows, hq, hk, k0, keys, strided, _ = case
    q8, k8, v8, v_scale = _attn_reference(case)[:4]
    view = ops.Kv8CacheView(k8.cuda(), v8.cuda(), v_scale.cuda())
    obuf = None
    if strided:
        qbuf = torch.full((rows, hq * HD + 48), 0x7F, dtype=torch.uint8, device="cuda")
        obuf = torch.full((rows, hq * HD + 24), 7.0, dtype=BF, device="cuda")
        qg, og = qbuf[:, 16:16 + hq * HD].view(rows, hq, HD), obuf[:, 8:8 + hq * HD].view(rows, hq, HD)
        qg.copy_(q8)
    else:
        qg, og = q8.cuda(), None
    if poison:          # the WHOLE workspace, arrival counters included: nothing it held may matter
        need = ops.attention_kv8_split_plan(rows, hq, k0, k0 + keys, splits)["workspace_bytes"]
        ops._kv8_split_workspace(qg.device, need).view(torch.uint8).fill_(0xFF)
    out, lse = ops.attention_kv8(qg, view, k0 + keys, out=og, return_lse=True, kv_start=k0, splits=splits)
    return out, lse, obuf


@pytest.mark.parametrize("case,splits", CASES, ids=lambda c: "-".join(str(int(x)) for x in c) if isinstance(c, tuple) else f"s{c}")
def test_split_against_fp64(ops, case, splits):
    rows, hq, _, k0, keys, strided, _ = case
    out64, lse64, emu64 = _attn_reference(case)[4:]
    plan = ops.attention_kv8_split_plan(rows, hq, k0, k0 + keys, splits)
    assert plan["chunks"] == min(splits, -(-keys // 64)) > 1
    out, lse, obuf = _launch(ops, case, splits)
    if strided:
        assert bool((obuf[:, :8] == 7.0).all()) and bool((obuf[:, 8 + hq * HD:] == 7.0).all()), "columns outside the output window were written"
    rel, rel_emu = rel_l2(out.cpu(), out64), rel_l2(emu64, out64)
    lse_err = (lse.cpu().double() - lse64).abs().max().item()
    print(f"attention_kv8 split {case} x{splits}: rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}, lse err {lse_err:.2e}")
    assert rel <= 1.25 * rel_emu + 1e-3 and lse_err <= 2e-3          # (NaN compares false)


def test_exactness_and_reuse(ops):
    # one chunk through the new entry point (4 splits of 63 keys clamp to 1) is the unsplit launch, bit for bit
    one = (33, 2, 2, 0, 63, False, False)
    assert ops.attention_kv8_split_plan(33, 2, 0, 63, 4)["workspace_bytes"] == 0
    a, la, _ = _launch(ops, one, 4, poison=False)
    b, lb, _ = _launch(ops, one, 1, poison=False)
    assert torch.equal(a, b) and torch.equal(la, lb)
    # the same split launch twice, the second on the workspace the first left behind: the merge order is the chunk order
    case = (300, 4, 2, 0, 64 * 5 + 5, False, False)
    a, la, _ = _launch(ops, case, 3)
    b, lb, _ = _launch(ops, case, 3, poison=False)
    assert torch.equal(a, b) and torch.equal(la, lb)


def test_rollout_split(ops, monkeypatch):
    """With chunks of one tile allowed the tiny rollout's forwards split; the rule and the integer trace are test_rollout_kv8's.
    `kv8_split=False` under the same option value is the run without the option, bit for bit."""
    parent = _rollout(kv_cache_dtype="fp8_e4m3")[0]
    with ops.option_scope("attn_kv8_split_min_tiles", 1):
        out8, trace8, fx = _rollout(kv_cache_dtype="fp8_e4m3")[:3]
        off = _rollout(kv_cache_dtype="fp8_e4m3", kv8_split=False)[0]
        keys = max(t[2] for t in trace8)                                  # local_end of the last block: 3 frames x 24 tokens, 2 heads
        chunks = ops.attention_kv8_split_plan(3 * 24, 2, 0, keys)["chunks"]
    assert chunks > 1, (keys, chunks)
    assert trace8 == [tuple(r) for r in fx["trace"].tolist()]
    assert torch.equal(off, parent)
    assert not torch.equal(out8, parent), "the model did not take the split launch"
    d8, d_emu = rel_l2(out8, fx["out"]), rel_l2(_emulated_oracle_rollout(fx, monkeypatch), fx["out"])
    print(f"rollout_tiny, split 8-bit attention vs the oracle rollout: {d8:.3e}; oracle with emulated 8-bit attention {d_emu:.3e}")
    assert d8 <= 1.5 * d_emu

"""The ring cache's multi-session launches on the GPU (include/inferix_hip_kv8_ring_sessions.h): the grouped attention of a set against
the single grouped launches (bit for bit) and against fp64 attention over the dequantised bytes (the rule of
test_hip_attn_kv8_ring.py); the fused append's scales against the stated rule, its bytes against e4m3(v / scale) and the single ring
append; one ragged model forward against the per-sample path."""
import pytest
import torch

import wan_oracle as O
from test_hip_attn_kv8 import BF, EPS, GRID_HW, HD, START_FRAME, code_distance, e4m3, ops  # noqa: F401 (ops: fixture)
from test_hip_attn_kv8_ring import _case
from util import rel_l2

pytestmark = pytest.mark.gpu
#        G  hq hk items (rows, kv_len)
SETS = [(100, 4, 2, [(1, 100), (65, 300), (300, 250), (0, 100)]),          # every group has a partial tile
        (24, 2, 1, [(1, 72), (33, 24), (70, 100), (5, 48), (256, 200), (2, 25), (40, 96), (17, 71), (257, 130)])]      # two launches


@pytest.mark.parametrize("G,hq,hk,items", SETS, ids=["G100", "G24x9"])
def test_attention_kv8_grouped_multi(ops, G, hq, hk, items):
    call, alone, want, emu = [], [], [], []
    for i, (rows, kv_len) in enumerate(items):
        q8, k8, v8, scale, out64, _, emu64 = _case(max(rows, 1), hq, hk, G, kv_len, draw=i)      # 0x7F (NaN) in every slot past kv_len
        view = ops.Kv8RingView(k8.cuda(), v8.cuda(), scale.cuda(), G)
        call.append((q8.cuda()[:rows], view, kv_len, torch.full((max(rows, 1), hq, HD), 7.0, dtype=BF, device="cuda")[:rows]))
        alone.append(ops.attention_kv8_grouped(call[-1][0], view, kv_len) if rows else call[-1][3])      # (no rows: nothing to launch alone)
        want.append(out64[:rows]), emu.append(emu64[:rows])
    ops.attention_kv8_grouped_multi(call, hq)
    for i, (it, one) in enumerate(zip(call, alone)):
        assert torch.equal(it[3], one), f"item {i} {items[i]} differs from its single launch"
    got, want, emu = torch.cat([it[3].cpu() for it in call]), torch.cat(want), torch.cat(emu)
    rel, rel_emu = rel_l2(got, want), rel_l2(emu, want)
    print(f"attention_kv8_grouped_multi G {G}: {got.shape[0] * hq} softmax rows, rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}")
    assert got.shape[0] * hq >= 64 and rel <= 1.25 * rel_emu + 1e-3


def _rule(amax):
    """The smallest power of two s with max(amax, 2^-20) <= 448 s, by enumeration in float64."""
    s = 2.0 ** torch.arange(-40, 41).double()
    return s[(amax.double().clamp_min(2.0 ** -20)[..., None] <= 448 * s).int().argmax(-1)].float()


@pytest.mark.parametrize("G", [24, 100])
def test_ring_append_multi(ops, G):
    """A one-frame sink and a ring of four frames per item.  Item 0 fills the sink and the first ring frame, item 1 starts a lap on and
    straddles the ring's end, item 2 is one frame mid-ring.  Planted in item 1: a slab of zeros, an amax of exactly 7 * 2^2 (negative),
    and the next bf16 above it in the slab's last row."""
    from inferix_amd import _hip
    heads, base, ring, SENT = 2, G, 4 * G, -3.0
    dim, cap, q_scale = heads * HD, 5 * G, ops.attn_q_prescale(HD)[0]
    freqs = torch.view_as_real(O.rope_freqs(HD)).contiguous().cuda()
    g = torch.Generator().manual_seed(G)
    wq, wk = ((1 + 0.1 * torch.randn(dim, generator=g)).to(BF).cuda() for _ in range(2))
    new_view = lambda table: ops.Kv8RingView(*(torch.full((cap, heads, HD), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)), table.cuda(), G)
    call, want = [], []
    for i, (start, frames) in enumerate([(0, 2), (base + ring + 2 * G, 3), (base + G, 1)]):
        qkv = (torch.randn(frames * G, 3 * dim, generator=g) * 2).to(BF)
        v = qkv[:, 2 * dim:].view(frames, G, heads, HD)          # (a view: planting writes qkv)
        if i == 1:
            v[0, :, 0] = 0
            v[1, G // 2, 1, 5], v[2, G - 1, 0, 127] = -28.0, 28.125
        slots = torch.tensor([p if p < base else base + (p - base) % ring for p in range(start, start + frames * G)])
        scale = _rule(v.float().abs().amax(dim=(1, 3)))          # [frames, heads]
        if i == 1:
            assert scale[0, 0] == 2.0 ** -28 and scale[1, 1] == 2.0 ** -4 and scale[2, 0] == 2.0 ** -3 and slots[-1] == base + G - 1
        table = torch.full((cap // G, heads), SENT)
        table[slots[::G] // G] = scale
        rope = ops.RopeGridSpec(freqs, START_FRAME + i, *GRID_HW, q_scale=q_scale)
        view, ref = new_view(torch.full((cap // G, heads), SENT)), new_view(table)
        q_ref = ops.rmsnorm_rope_kv8_append_ring(qkv.cuda(), wq, wk, EPS, rope, ref, base, ring, start, dim)
        call.append((qkv.cuda(), rope, view, base, ring, start, torch.empty(frames * G, dim, dtype=torch.uint8, device="cuda")))
        want.append((table, e4m3(v.float() / scale.view(frames, 1, heads, 1)).view(-1, heads, HD), slots, ref, q_ref))
    ops.rmsnorm_rope_kv8_append_ring_multi(call, wq, wk, EPS, dim)
    for i, (it, (table, v8, slots, ref, q_ref)) in enumerate(zip(call, want)):
        view = it[2]
        assert torch.equal(view.v_scale.cpu(), table), (i, view.v_scale.cpu(), table)          # the rule exactly; sentinels elsewhere
        assert code_distance(view.v.cpu()[slots], v8).max() == 0, i
        assert torch.equal(it[6], q_ref) and torch.equal(view.k, ref.k) and torch.equal(view.v, ref.v), i
        rest = torch.ones(cap, dtype=torch.bool)
        rest[slots] = False
        assert rest.any() and all(bool((c.cpu()[rest] == 0xA5).all()) for c in (view.k, view.v)), "bytes outside the appended slots changed"
    with pytest.raises(_hip.HipKernelError, match=rf"code {_hip.IFX_EINVAL}\)"):
        ops.rmsnorm_rope_kv8_append_ring_multi([call[0], call[2][:5] + (base + G + 1,) + call[2][6:]], wq, wk, EPS, dim)


def test_ragged_forward_ring_multi_launches_equal_the_per_sample_path(monkeypatch):
    from inferix_amd import hip_ops
    from test_hip_kv8_ring_model import RingWorld
    from test_hip_ragged_forward import _cfg
    w = RingWorld(_cfg())
    calls, real = [], hip_ops.rmsnorm_rope_kv8_append_ring_multi
    monkeypatch.setattr(hip_ops, "rmsnorm_rope_kv8_append_ring_multi", lambda items, *a, **kw: (calls.append(len(items)), real(items, *a, **kw))[1])
    s_on, s_off = w.copy(), w.copy()
    on = w.ragged(s_on)
    assert calls == [3] * w.cfg.num_layers          # one append launch per layer for the three samples
    monkeypatch.setattr(w.m, "attn_multi", False)
    off = w.ragged(s_off)
    torch.cuda.synchronize()
    assert len(calls) == w.cfg.num_layers and torch.isfinite(on.float()).all() and torch.equal(on, off)
    assert all(torch.equal(a, b) for a, b in zip(w.caches(s_on), w.caches(s_off)))
    tables = lambda s: [s.kvm.request_to_kv_caches[r.request_id].views[f"layer_{l}"][1].v_scale for r in s.reqs for l in range(w.cfg.num_layers)]
    assert all(torch.equal(a, b) for a, b in zip(tables(s_on), tables(s_off)))

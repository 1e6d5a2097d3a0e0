"""The 8-bit ring cache's kernels on the GPU (include/inferix_hip_kv8_ring.h): the grouped attention — a V scale per group of slots —
against fp64 attention over the dequantised bytes (yardstick: the fp64 emulation that rounds P to e4m3, the rule of
test_hip_attn_kv8.py), and the ring append's bytes against the fp32 restatement of test_hip_attn_kv8.py."""
import math

import pytest
import torch

import wan_oracle as O
from attn_window_util import plant
from test_hip_attn_kv8 import BF, EPS, F8, GRID_HW, HD, Q_SCALE, START_FRAME, _restate, code_distance, e4m3, ops  # noqa: F401 (ops: fixture)
from util import rel_l2

pytestmark = pytest.mark.gpu
#         rows hq hk   G  kv_len
SHAPES = [(1, 2, 1, 24, 72),               # a group smaller than a tile
          (65, 12, 12, 100, 300),          # a partial tile in every group
          (300, 12, 2, 128, 448),          # GQA, two row tiles, ragged last tile, last group partial
          (300, 2, 2, 1560, 4680)]         # the real frame: 24.375 tiles


def _case(rows, hq, hk, G, kv_len, equal=False, draw=0):
    """(q8, k8, v8 bytes, scale table, out64, lse64, emu64): inputs as test_hip_attn_kv8._attn_reference's, the V bytes of group g
    quantised with scale[g] (non-monotone powers of two 2^-3 .. 2^4, distinct per head), 0x7F (NaN) in every slot past kv_len."""
    cap = (-(-kv_len // G) + 1) * G
    g = torch.Generator().manual_seed(1000 * rows + kv_len + 7919 * draw)
    q = torch.randn(rows, hq, HD, generator=g).to(BF)
    k, v = (torch.randn(cap, hk, HD, generator=g).to(BF) for _ in range(2))
    plant(q, k, v, 0, kv_len)
    scale = torch.tensor([[0.5 if equal else 2.0 ** ((5 * i + 3 * c) % 8 - 3) for c in range(hk)] for i in range(cap // G)])
    per_slot = scale.repeat_interleave(G, dim=0).view(cap, hk, 1)
    q8, k8, v8 = e4m3(q.float() * Q_SCALE), e4m3(k), e4m3(v.float() / per_slot)
    k8[kv_len:], v8[kv_len:] = 0x7F, 0x7F
    deq, gsz = (lambda b: b.view(F8).double()), hq // hk
    qd = deq(q8).transpose(0, 1)
    kd = deq(k8)[:kv_len].repeat_interleave(gsz, dim=1).transpose(0, 1)
    vd = (deq(v8)[:kv_len] * per_slot[:kv_len].double()).repeat_interleave(gsz, dim=1).transpose(0, 1)
    s = qd @ kd.transpose(1, 2)
    mx = s.max(-1, keepdim=True).values
    p = torch.exp2(s - mx)
    l = p.sum(-1, keepdim=True)
    emu64 = (((p * 128).float().to(F8).double() @ vd) / (l * 128)).transpose(0, 1)
    return q8, k8, v8, scale, ((p @ vd) / l).transpose(0, 1), (mx + torch.log2(l)).squeeze(-1) * math.log(2), emu64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: "-".join(str(x) for x in c))
def test_attention_kv8_grouped(ops, shape):
    """The rule compares two error LEVELS (the kernel rounds P on the grid of its lazy maximum, the emulation on the true maximum's:
    the same distribution, other draws), so each is taken over at least 64 (row, head) softmax rows: a shape with fewer is launched
    on as many independent inputs as that takes, and the rows are pooled.  One draw of (1, 2, 1, 24, 72) is ONE row whose error is a
    handful of roundings (its planted head is exact): measured 8.36e-3 against 5.04e-3, and 8.36e-3 too from an fp64 emulation on the
    kernel's own grid."""
    rows, hq, hk, G, kv_len = shape
    plan = ops.attention_kv8_grouped_plan(rows, hq, G, kv_len)
    assert plan["tiles_per_group"] == -(-G // 64) and plan["key_tiles"] == (kv_len // G) * plan["tiles_per_group"] + -(-(kv_len % G) // 64)
    got, want, emu, lse_err = [], [], [], 0.0
    for draw in range(-(-64 // (rows * hq))):
        q8, k8, v8, scale, out64, lse64, emu64 = _case(*shape, draw=draw)
        view = ops.Kv8RingView(k8.cuda(), v8.cuda(), scale.cuda(), G)
        out, lse = ops.attention_kv8_grouped(q8.cuda(), view, kv_len, return_lse=True)
        got.append(out.cpu()), want.append(out64), emu.append(emu64)
        lse_err = max(lse_err, (lse.cpu().double() - lse64).abs().max().item())
    rel, rel_emu = rel_l2(torch.cat(got), torch.cat(want)), rel_l2(torch.cat(emu), torch.cat(want))
    print(f"attention_kv8_grouped {shape}: rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}, lse err {lse_err:.2e}")
    assert rel <= 1.25 * rel_emu + 1e-3 and lse_err <= 2e-3          # (NaN compares false)


def test_equal_scales_and_whole_tiles_give_the_flat_kernels_bits(ops):
    q8, k8, v8, scale = _case(300, 4, 2, 128, 448, equal=True)[:4]
    ring = ops.Kv8RingView(k8.cuda(), v8.cuda(), scale.cuda(), 128)
    got = ops.attention_kv8_grouped(q8.cuda(), ring, 448, return_lse=True)
    want = ops.attention_kv8(q8.cuda(), ops.Kv8CacheView(ring.k, ring.v, scale[0].cuda()), 448, return_lse=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("frames,G", [(2, 24), (3, 100)])
def test_ring_append_bytes(ops, frames, G):
    """A one-frame sink and a ring of four frames; the rows start more than a lap on, 7 slots before a group boundary, and straddle
    the ring's end."""
    from inferix_amd import _hip
    heads, rows, base, ring = 2, frames * G, G, 4 * G
    dim, cap, start = heads * HD, base + ring, base + ring + (4 - frames) * G + G - 7
    g = torch.Generator().manual_seed(G)
    qkv = (torch.randn(rows, 3 * dim, generator=g) * 2).to(BF)
    wq, wk = ((1 + 0.1 * torch.randn(dim, generator=g)).to(BF) for _ in range(2))
    scale = torch.tensor([[2.0 ** ((i + c) % 3 - 1) for c in range(heads)] for i in range(cap // G)])
    slots = torch.tensor([p if p < base else base + (p - base) % ring for p in range(start, start + rows)])
    assert slots.max() == cap - 1 and slots.min() == base and slots[0] % G == G - 7
    q_scale = ops.attn_q_prescale(HD)[0]
    q, k, v = qkv.split(dim, dim=1)
    want = {"q": _restate(q, wq, heads, q_scale, 0), "k": _restate(k, wk, heads, 1.0, 0),
            "v": e4m3(v.float().view(rows, heads, HD) / scale[slots // G].view(rows, heads, 1)).view(rows, dim)}
    kc, vc = (torch.full((cap, heads, HD), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    rope = ops.RopeGridSpec(torch.view_as_real(O.rope_freqs(HD)).contiguous().cuda(), START_FRAME, *GRID_HW, q_scale=q_scale)
    view = ops.Kv8RingView(kc, vc, scale.cuda(), G)
    q8 = ops.rmsnorm_rope_kv8_append_ring(qkv.cuda(), wq.cuda(), wk.cuda(), EPS, rope, view, base, ring, start, dim)
    got = {"q": q8.cpu(), "k": kc.cpu()[slots].view(rows, dim), "v": vc.cpu()[slots].view(rows, dim)}
    for name in ("q", "k", "v"):
        d = code_distance(got[name], want[name])
        frac = (d > 0).float().mean().item()
        print(f"ring append {frames} x {G} {name}: max code distance {d.max().item()}, differing {frac:.5f}")
        assert d.max() <= (0 if name == "v" else 1) and frac <= 0.005, (name, d.max(), frac)
    rest = torch.ones(cap, dtype=torch.bool)
    rest[slots] = False
    assert not rest[:base].logical_not().any() and all(bool((c.cpu()[rest] == 0xA5).all()) for c in (kc, vc)), "bytes outside the appended slots changed"
    with pytest.raises(_hip.HipKernelError, match=rf"code {_hip.IFX_EINVAL}\)"):          # more rows than the ring holds
        ops.rmsnorm_rope_kv8_append_ring(qkv.cuda(), wq.cuda(), wk.cuda(), EPS, rope, view, base, rows - G, start, dim)

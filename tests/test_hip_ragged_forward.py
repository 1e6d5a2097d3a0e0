"""A forward whose samples are at different positions of their videos (per-sample `current_start` / cache-meta lists): three requests at
blocks 0, 1 and 3 — the first on its first forward (cross cache uninitialised), the last past the local-attention window and evicting —
against the same requests run alone, against the CPU oracle at each sample's own position, and with the multi launch on and off."""
import pytest
import torch

import wan_oracle as O
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POSITIONS = (0, 1, 3)            # the block each request is at
NF = 3


@pytest.fixture(autouse=True)
def _options_back():
    from inferix_amd import hip_ops as ops
    yield
    ops.set_option("attn_variant", 0)


def _cfg():
    return O.tiny_config(local_attn_size=6, sink_size=1)        # a window of two blocks: block 2 and later evict


def _inputs(cfg):
    """Per request: the clean latents of its history blocks, the noisy block it is at, its prompt; made once, never modified."""
    g = torch.Generator().manual_seed(27)
    lat = lambda: torch.randn(1, 16, NF, cfg.latent_h, cfg.latent_w, generator=g).to(BF)
    reqs = []
    for r, p in enumerate(POSITIONS):
        n_text = (5, 9, cfg.text_len)[r]
        reqs.append(dict(history=[lat() for _ in range(p)], x=lat(), prompt=torch.randn(n_text, cfg.text_dim, generator=g).to(BF)))
    return reqs


class World:
    """One model and, per `copy()`, the three requests with their histories run (solo forwards at t = 0), ready for the forward under
    test.  Every copy goes through the same launches, so the copies' caches are identical."""

    def __init__(self, cfg):
        from inferix_amd.wan import HipCausalWanModel
        self.cfg, self.W = cfg, O.init_weights(cfg, seed=0)
        self.m = HipCausalWanModel(patch_size=cfg.patch_size, text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim, ffn_dim=cfg.ffn_dim,
                                   freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim, num_heads=cfg.num_heads,
                                   num_layers=cfg.num_layers, local_attn_size=cfg.local_attn_size, sink_size=cfg.sink_size, eps=cfg.eps)
        self.m.load_state_dict(self.W)
        self.inp = _inputs(cfg)
        self.N = NF * cfg.frame_seqlen
        self.t0 = torch.zeros(1, NF, dtype=torch.int64)
        self.t = torch.full((1, NF), 500, dtype=torch.int64)

    def fresh(self, n=3):
        from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
        kvm = KVCacheManager("cuda")
        reqs = [KVCacheRequest(f"r{i}") for i in range(n)]
        size = self.cfg.local_attn_size * self.cfg.frame_seqlen
        for blk in self.m.blocks:
            for r in reqs:
                blk.kv_cache_manager.allocate_kv_cache(kv_cache_manager=kvm, kv_cache_request=r, sequence_length=size, dtype=BF)
                blk.kv_cache_manager.allocate_crossattn_cache(kv_cache_manager=kvm, kv_cache_request=r, crossattn_length=self.cfg.text_len, dtype=BF)
        L = self.cfg.num_layers
        kv = [[{"global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])} for _ in range(L)] for _ in reqs]
        cross = [[{"is_init": False} for _ in range(L)] for _ in reqs]
        return SimpleState(kvm, reqs, kv, cross)

    def solo(self, s, r, x, t, start):
        return self.m(x=x.cuda(), t=t.cuda(), context=[self.inp[r]["prompt"].cuda()], kv_cache_meta=s.kv[r], crossattn_cache_meta=s.cross[r],
                      current_start=start, kv_cache_manager=s.kvm, kv_cache_requests=[s.reqs[r]])

    def copy(self):
        s = self.fresh()
        for r, it in enumerate(self.inp):
            for b, h in enumerate(it["history"]):
                self.solo(s, r, h, self.t0, b * self.N)
        return s

    def ragged(self, s):
        return self.m(x=torch.cat([it["x"] for it in self.inp]).cuda(), t=self.t.expand(3, NF).contiguous().cuda(),
                      context=[it["prompt"].cuda() for it in self.inp], kv_cache_meta=s.kv, crossattn_cache_meta=s.cross,
                      current_start=[p * self.N for p in POSITIONS], kv_cache_manager=s.kvm, kv_cache_requests=s.reqs)

    def caches(self, s):
        """The rows written so far of every self-attention cache (the storage behind them is uninitialised) and the cross caches."""
        out = []
        for i, r in enumerate(s.reqs):
            for l in range(self.cfg.num_layers):
                le = int(s.kv[i][l]["local_end_index"])
                out.append(s.kvm.get_raw(r, f"layer_{l}").flatten(1, 2)[:, :le].clone())
                out.append(s.kvm.get_raw(r, f"crossattn_layer_{l}").clone())
        return out


class SimpleState:
    def __init__(self, kvm, reqs, kv, cross):
        self.kvm, self.reqs, self.kv, self.cross = kvm, reqs, kv, cross


@pytest.fixture(scope="module")
def world():
    return World(_cfg())


@pytest.mark.parametrize("variant", [0, 7])
def test_ragged_samples_against_their_solo_forwards(world, variant):
    """Host integers exactly; numerics within 2 x the distance between the parent's own uniform batch and its solo forwards.

    Measured on an MI355X (profiles/r27_sessions.md): the yardstick and all three distances are 0 under both variants, so
    the comparison is torch.equal."""
    from inferix_amd import hip_ops as ops
    w, m = world, world.m
    ops.set_option("attn_variant", variant)       # 0: these small items launch one by one; 7: the multi launch
    # yardstick: code this change does not touch — the three requests at ONE position as a uniform batch against three solo forwards
    su, ss = w.fresh(), w.fresh()
    kvu = [{"global_end_index": torch.tensor([0]), "local_end_index": torch.tensor([0])} for _ in range(w.cfg.num_layers)]
    uniform = m(x=torch.cat([it["x"] for it in w.inp]).cuda(), t=w.t.expand(3, NF).contiguous().cuda(),
                context=[it["prompt"].cuda() for it in w.inp], kv_cache_meta=kvu, crossattn_cache_meta=su.cross[0], current_start=0,
                kv_cache_manager=su.kvm, kv_cache_requests=su.reqs)
    alone0 = [w.solo(ss, r, w.inp[r]["x"], w.t, 0) for r in range(3)]
    yard = max(rel_l2(uniform[r:r + 1].cpu(), alone0[r].cpu()) for r in range(3))
    # the same requests, each at its own position: solo ...
    s1, s2 = w.copy(), w.copy()
    assert [int(m_[0]["local_end_index"]) for m_ in s1.kv] == [0, w.N, 2 * w.N]      # block 3 starts from a full window
    assert [c[0]["is_init"] for c in s1.cross] == [False, True, True]
    m.index_trace = []
    alone = [w.solo(s1, r, w.inp[r]["x"], w.t, POSITIONS[r] * w.N) for r in range(3)]
    trace_solo, m.index_trace = m.index_trace, []
    # ... and in one ragged forward
    rag = w.ragged(s2)
    trace_ragged, m.index_trace = m.index_trace, None
    torch.cuda.synchronize()
    assert trace_ragged == trace_solo and len(trace_solo) == 3
    assert [t[0] for t in trace_solo] == [p * w.N for p in POSITIONS]
    assert trace_solo[2][2] == 2 * w.N and trace_solo[2][1] == 4 * w.N                  # evicting: the window stays full
    for a, b in zip(s1.kv + s1.cross, s2.kv + s2.cross):
        assert [{k: int(v) for k, v in d.items()} for d in a] == [{k: int(v) for k, v in d.items()} for d in b]
    assert all(d["is_init"] for c in s2.cross for d in c)
    dist = [rel_l2(rag[r:r + 1].cpu(), alone[r].cpu()) for r in range(3)]
    print(f"RAGGED|variant {variant}|yardstick (uniform batch vs solo) {yard:.3e}|ragged vs solo {' '.join(f'{d:.3e}' for d in dist)}")
    for r in range(3):
        if yard == 0.0:
            assert torch.equal(rag[r:r + 1], alone[r]), (r, dist[r])
        else:
            assert dist[r] <= 2 * yard, (r, dist[r], yard)
    if yard == 0.0:        # then the caches the two ways left behind are the same bits too
        assert all(torch.equal(a, b) for a, b in zip(w.caches(s1), w.caches(s2)))


@pytest.mark.parametrize("variant", [0, 7])
def test_ragged_samples_against_the_oracle_at_their_own_positions(world, variant):
    """The bound of tests/test_hip_model.py for a solo forward: as close to the oracle (bf16 SDPA) and to its exact-attention run as
    1.25 x the distance between those two + 5e-4 — per sample, each with its own history, position and prompt."""
    from inferix_amd import hip_ops as ops
    w, cfg = world, world.cfg
    ops.set_option("attn_variant", variant)
    rag = w.ragged(w.copy()).cpu()
    for r, it in enumerate(w.inp):
        flows = {}
        for impl in ("sdpa", "math"):
            st = O.CacheState.allocate(cfg, 1, BF)
            for b, h in enumerate(it["history"]):
                O.model_forward(w.W, cfg, h, w.t0, [it["prompt"]], st, b * w.N, attn_impl=impl)
            flows[impl] = O.model_forward(w.W, cfg, it["x"], w.t, [it["prompt"]], st, POSITIONS[r] * w.N, attn_impl=impl)
        floor = rel_l2(flows["sdpa"], flows["math"])
        r_ref, r_exact = rel_l2(rag[r:r + 1], flows["sdpa"]), rel_l2(rag[r:r + 1], flows["math"])
        print(f"RAGGED|variant {variant}|sample {r} at block {POSITIONS[r]}: floor {floor:.3e}; HIP vs exact {r_exact:.3e}; HIP vs oracle {r_ref:.3e}")
        assert r_ref <= 1.25 * floor + 5e-4 and r_exact <= 1.25 * floor + 5e-4, (r, floor, r_ref, r_exact)


@pytest.mark.parametrize("variant", [6, 7])
def test_multi_launch_on_and_off_give_the_same_bits(world, variant, monkeypatch):
    from inferix_amd import hip_ops as ops
    w, m = world, world.m
    ops.set_option("attn_variant", variant)
    calls = []
    real = ops.attention_multi
    monkeypatch.setattr(ops, "attention_multi", lambda items, *a, **kw: (calls.append(len(items)), real(items, *a, **kw))[1])
    s_on, s_off = w.copy(), w.copy()
    assert m.attn_multi is True
    on = w.ragged(s_on)
    assert calls == [3] * w.cfg.num_layers          # one launch per layer for the three samples
    monkeypatch.setattr(m, "attn_multi", False)
    off = w.ragged(s_off)
    assert len(calls) == w.cfg.num_layers
    torch.cuda.synchronize()
    assert torch.equal(on, off)
    assert all(torch.equal(a, b) for a, b in zip(w.caches(s_on), w.caches(s_off)))


def test_ragged_lists_are_checked(world):
    w = world
    s = w.fresh()
    kw = dict(x=torch.cat([it["x"] for it in w.inp]).cuda(), t=w.t.expand(3, NF).contiguous().cuda(), context=[it["prompt"].cuda() for it in w.inp],
              kv_cache_manager=s.kvm, kv_cache_requests=s.reqs)
    with pytest.raises(ValueError, match="3 requests need 3 entries"):
        w.m(**kw, kv_cache_meta=s.kv, crossattn_cache_meta=s.cross, current_start=[0, 0])
    with pytest.raises(ValueError, match="one dict per layer"):
        w.m(**kw, kv_cache_meta=[k[:1] for k in s.kv], crossattn_cache_meta=s.cross, current_start=[0, 0, 0])
    cp, w.m.cp = w.m.cp, object()
    try:
        with pytest.raises(NotImplementedError, match="sequence parallelism"):
            w.m(**kw, kv_cache_meta=s.kv, crossattn_cache_meta=s.cross, current_start=[0, 0, 0])
    finally:
        w.m.cp = cp

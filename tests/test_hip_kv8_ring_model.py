"""kv_cache_dtype='fp8_e4m3_ring' through the model: the tiny rollout with a rolling window (local_attn_size=6, sink_size=1) against the
oracle rollout with the emulated format, and a ragged forward whose samples stand at different blocks against their solo forwards."""
import pytest
import torch

import wan_oracle as O
from test_hip_attn_kv8 import BF, F8, Q_SCALE, e4m3
from test_hip_ragged_forward import POSITIONS, World, _cfg
from util import rel_l2

pytestmark = pytest.mark.gpu
LOCAL = dict(local_attn_size=6, sink_size=1)


def _rollout(fx, prior=False, **model_kw):
    """The rolling tiny rollout through CausalInferencePipeline: (latents, integer trace).  `prior`: a clip with 4 x the noise first."""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    from test_hip_model import _pipeline
    cfg = O.tiny_config(**LOCAL)
    m, gen, args = _pipeline(cfg, O.init_weights(cfg, seed=0), fx["steps"].tolist(), float(fx["shift"]), **model_kw)
    pe = fx["prompt_embeds"].cuda()
    pipe = CausalInferencePipeline(args, "cuda", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
    kvm, reqs = KVCacheManager("cuda"), [KVCacheRequest("req0")]
    for scale in ([4.0] if prior else []) + [1.0]:
        m.index_trace = []
        out = pipe.inference(noise=(fx["noise"].float() * scale).to(BF).cuda(), text_prompts=["x"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                             initial_latent=None, decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False,
                             renoise=[fx[f"renoise_{i}"] for i in range(int(fx["num_renoise"]))])
    return out.cpu(), m.index_trace


def _emulated_oracle_rollout(fx, monkeypatch):
    """The wan_oracle rollout with its self-attention replaced by the fp64 emulation of the ring format: q, K and P rounded to e4m3, V
    to e4m3 with a scale per frame and head, exp2(ceil(log2(max(amax, 2^-20) / 448))) of the frame's own rows (the window is whole
    frames in any order).  Cross-attention (text_len keys) keeps the oracle's own function."""
    cfg, real = O.tiny_config(**LOCAL), O.attention

    def emulated(q, k, v, impl="sdpa"):
        if k.shape[1] == cfg.text_len:
            return real(q, k, v, impl)
        B, L, H, D = v.shape
        amax = v.float().abs().view(B, L // cfg.frame_seqlen, cfg.frame_seqlen, H, D).amax(dim=(2, 4), keepdim=True)
        sc = torch.exp2(torch.ceil(torch.log2(amax.clamp_min(2.0 ** -20) / 448))).expand(-1, -1, cfg.frame_seqlen, -1, -1).reshape(B, L, H, 1)
        deq = lambda x: e4m3(x).view(F8).double().transpose(1, 2)             # [B, H, L, 128]
        qd, kd, vd = deq(q.float() * Q_SCALE), deq(k), deq(v.float() / sc) * sc.transpose(1, 2).double()
        s = qd @ kd.transpose(-1, -2)
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        return (((p * 128).float().to(F8).double() @ vd) / (128 * p.sum(-1, keepdim=True))).transpose(1, 2).to(q.dtype).contiguous()
    monkeypatch.setattr(O, "attention", emulated)
    out, _ = O.inference(O.init_weights(cfg, seed=0), cfg, fx["noise"], list(fx["prompt_embeds"]), fx["steps"].tolist(), shift=float(fx["shift"]),
                         renoise=[fx[f"renoise_{i}"] for i in range(int(fx["num_renoise"]))], num_frame_per_block=3,
                         state=O.CacheState.allocate(cfg, 1, BF))
    return out


def test_rolling_rollout_kv8_ring(monkeypatch):
    """Integer cache state = the bf16 run's = the reference trace (the ring moves no logical index); latents within 1.5 x the distance
    the oracle rollout itself shows with the emulated format (the rule of test_rollout_kv8); a clip does not depend on the clip
    before it; 'fp8_e4m3' still refuses the rolling window."""
    from fixture_io import golden
    from test_hip_model import build
    fx = golden("rollout_tiny_local.npz")
    out8, trace8 = _rollout(fx, kv_cache_dtype="fp8_e4m3_ring")
    out16, trace16 = _rollout(fx)
    assert trace8 == trace16 == [tuple(r) for r in fx["trace"].tolist()]
    d8, d_emu = rel_l2(out8, fx["out"]), rel_l2(_emulated_oracle_rollout(fx, monkeypatch), fx["out"])
    print(f"rollout_tiny_local vs the oracle rollout: fp8_e4m3_ring cache {d8:.3e}; oracle with the emulated format {d_emu:.3e}; bf16 cache "
          f"{rel_l2(out16, fx['out']):.3e}")
    assert d8 <= 1.5 * d_emu
    assert torch.equal(_rollout(fx, prior=True, kv_cache_dtype="fp8_e4m3_ring")[0], out8), "a clip depends on the clip before it"
    with pytest.raises(NotImplementedError, match="rolling eviction"):
        build(O.tiny_config(**LOCAL), O.init_weights(O.tiny_config(**LOCAL), seed=0), kv_cache_dtype="fp8_e4m3")


class RingWorld(World):
    """test_hip_ragged_forward's World on the ring format: the same requests and positions, uint8 self-attention caches."""

    def __init__(self, cfg):
        from test_hip_model import build
        super().__init__(cfg)
        self.m = build(cfg, self.W, kv_cache_dtype="fp8_e4m3_ring")

    def fresh(self, n=3):
        from inferix_amd.kvcache_manager import KVCacheManager
        s = super().fresh(n)
        s.kvm = KVCacheManager("cuda")                # the same allocations, the self-attention caches in bytes
        for blk in self.m.blocks:
            for r in s.reqs:
                blk.kv_cache_manager.allocate_kv_cache(kv_cache_manager=s.kvm, kv_cache_request=r, dtype=torch.uint8,
                                                       sequence_length=self.cfg.local_attn_size * self.cfg.frame_seqlen)
                blk.kv_cache_manager.allocate_crossattn_cache(kv_cache_manager=s.kvm, kv_cache_request=r, crossattn_length=self.cfg.text_len, dtype=BF)
        return s


def test_ragged_samples_equal_their_solo_forwards_kv8_ring():
    """Three samples at blocks 0, 1 and 3 — the last past its second eviction, its ring turned — in one ragged forward: each equals its
    own B = 1 forward bit for bit, and so do the caches and the index states."""
    w = RingWorld(_cfg())
    s1, s2 = w.copy(), w.copy()
    alone = [w.solo(s1, r, w.inp[r]["x"], w.t, POSITIONS[r] * w.N) for r in range(3)]
    rag = w.ragged(s2)
    torch.cuda.synchronize()
    ring = s2.kvm.request_to_kv_caches["r2"].views["layer_0"][1]
    assert type(ring).__name__ == "Kv8RingView" and ring.ring_offset == (2 * w.N) % (5 * w.cfg.frame_seqlen)      # two evictions of a block
    assert [int(m_[0]["local_end_index"]) for m_ in s2.kv] == [w.N, 2 * w.N, 2 * w.N]
    for r in range(3):
        assert torch.isfinite(rag[r].float()).all() and torch.equal(rag[r:r + 1], alone[r]), r
    assert all(torch.equal(a, b) for a, b in zip(w.caches(s1), w.caches(s2)))

"""The 8-bit (e4m3) KV cache on the GPU: the append kernel's bytes against an fp32 restatement, the FP8-MFMA attention kernel against
fp64 attention over the dequantised bytes (yardstick: an fp64 emulation that rounds P to e4m3), and a two-block model rollout."""
import math

import pytest
import torch

import wan_oracle as O
from attn_window_util import plant
from util import rel_l2

pytestmark = pytest.mark.gpu
BF, F8, HD, GRID_HW, START_FRAME, EPS = torch.bfloat16, torch.float8_e4m3fn, 128, (4, 6), 5, 1e-6


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops

def e4m3(x):      # the contract's conversion: clamp to +-448, round to nearest even; as bytes
    return x.float().clamp(-448, 448).to(F8).view(torch.uint8)


def code_distance(a, b):      # of two e4m3 byte tensors, in representable values (+0 and -0 coincide)
    o = lambda t: torch.where(t >= 128, -(t.int() - 128), t.int())
    return (o(a) - o(b)).abs()


def _restate(x, w, heads, scale, order):
    """fp32 restatement of RMSNorm -> bf16 -> x w -> bf16 -> rotation (complex128 -> fp32) -> x scale -> e4m3, the mean of squares
    summed in one of two orders."""
    rows, dim = x.shape
    xf = x.float()
    ss = xf.pow(2).sum(-1, keepdim=True) if order == 0 else xf.pow(2).view(rows, 8, dim // 8).sum(-1).flip(-1).cumsum(-1)[:, -1:]
    y = (xf * torch.rsqrt(ss / dim + EPS)).to(BF) * w
    h, w_ = GRID_HW
    f = -(-rows // (h * w_))
    pad = torch.zeros(f * h * w_, heads, HD)
    pad[:rows] = y.float().view(rows, heads, HD)
    rot = O.causal_rope_apply(pad[None], (f, h, w_), O.rope_freqs(HD), START_FRAME)[0, :rows]
    return e4m3(rot.reshape(rows, dim) * scale)


@pytest.mark.parametrize("rows,local_start,heads", [(1, 0, 2), (65, 37, 12), (300, 0, 12), (300, 37, 2)])
def test_append_bytes(ops, rows, local_start, heads):
    dim, cap = heads * HD, local_start + rows + 5
    g = torch.Generator().manual_seed(rows + local_start)
    qkv = (torch.randn(rows, 3 * dim, generator=g) * 2).to(BF)
    qkv[0, 2 * dim] = 1e4                                                     # a V value beyond 448 * v_scale saturates
    wq, wk = ((1 + 0.1 * torch.randn(dim, generator=g)).to(BF) for _ in range(2))
    v_scale = torch.tensor([2.0 ** (i % 3 - 1) for i in range(heads)])
    q_scale = ops.attn_q_prescale(HD)[0]
    q, k, v = qkv.split(dim, dim=1)
    want = {"q": _restate(q, wq, heads, q_scale, 0), "k": _restate(k, wk, heads, 1.0, 0),
            "v": e4m3(v.float().view(rows, heads, HD) / v_scale.view(1, heads, 1)).view(rows, dim)}
    # two fp32 summation orders of the restatement stay inside the cap the kernel is held to
    for name, x, w, s in (("q", q, wq, q_scale), ("k", k, wk, 1.0)):
        d = code_distance(want[name], _restate(x, w, heads, s, 1))
        assert d.max() <= 1 and (d > 0).float().mean() <= 0.005, (name, "restatement orders", d.max(), (d > 0).float().mean())
    kc, vc = (torch.full((cap, heads, HD), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
    rope = ops.RopeGridSpec(torch.view_as_real(O.rope_freqs(HD)).contiguous().cuda(), START_FRAME, *GRID_HW, q_scale=q_scale)
    view = ops.Kv8CacheView(kc, vc, v_scale.cuda())
    q8 = ops.rmsnorm_rope_kv8_append(qkv.cuda(), wq.cuda(), wk.cuda(), EPS, rope, view, local_start, dim)
    got = {"q": q8.cpu(), "k": kc[local_start:local_start + rows].cpu().view(rows, dim), "v": vc[local_start:local_start + rows].cpu().view(rows, dim)}
    for name in ("q", "k", "v"):
        d = code_distance(got[name], want[name])
        frac = (d > 0).float().mean().item()
        print(f"append rows {rows} start {local_start} heads {heads} {name}: max code distance {d.max().item()}, differing {frac:.5f}")
        assert d.max() <= (0 if name == "v" else 1) and frac <= 0.005, (name, d.max(), frac)
    assert want["v"][0, 0] == 0x7E                                            # 448: the saturated value
    for c in (kc, vc):
        assert bool((c[:local_start] == 0xA5).all()) and bool((c[local_start + rows:] == 0xA5).all()), "bytes outside the appended slots changed"


RING = 3
Q_SCALE = HD ** -0.5 * math.log2(math.e)         # what the append kernel folds into q (hip_ops.attn_q_prescale)
#        rows hq hk kv_start keys strided rising
CASES = [(1, 2, 2, 0, 1, False, False), (33, 2, 2, 0, 63, False, False), (256, 4, 2, 0, 64, False, False), (300, 2, 2, 0, 65, False, False),
         (33, 4, 2, 0, 200, False, False), (300, 4, 2, 0, 64 * (RING + 2) + 5, False, False), (33, 2, 2, 70, 200, False, False),
         (300, 4, 2, 0, 200, True, False), (33, 2, 2, 0, 64 * (RING + 2) + 5, False, True)]
_REFS = {}


def _attn_reference(case):
    """(q8, k8, v8 bytes, v_scale, out64, lse64, emu64) of a case, computed once.  out64 / lse64: fp64 attention over the DEQUANTISED
    bytes (scores are exponents of 2); emu64: the same with P = exp2(s - max + 7) rounded to e4m3 and the row sum from the unrounded P.
    Inputs at the model's scale, as in attn_window_util (q ~ N(0, 1) before Q_SCALE: a planted key scores ~65 in log2 units); the LSE
    error grows with the scores' magnitude, 1.1e-3 .. 2.2e-3 at planted scores of 130 .. 190 (profiles/r29_attn_kv8.md)."""
    if case in _REFS:
        return _REFS[case]
    rows, hq, hk, k0, keys, _, rising = case
    k1, cap = k0 + keys, k0 + keys + 3
    g = torch.Generator().manual_seed(1000 * rows + keys)
    q = torch.randn(rows, hq, HD, generator=g).to(BF)                        # the model's normalised q; the kernel gets e4m3(q * Q_SCALE)
    k, v = (torch.randn(cap, hk, HD, generator=g).to(BF) for _ in range(2))
    if rising:          # every q row shares u (|u|^2 = 32); key j gains 3 (j // 64) u / 32: scores rise by ~3 per tile
        u = 0.5 * torch.sign(torch.randn(HD, generator=g))
        q = (q.float() + u / Q_SCALE).to(BF)
        k = (k.float() + (3.0 / 32) * (torch.arange(cap) // 64).view(cap, 1, 1) * u).to(BF)
    else:
        plant(q, k, v, k0, k1)
    v_scale = torch.tensor([2.0, 0.5])[:hk]
    q8, k8, v8 = e4m3(q.float() * Q_SCALE), e4m3(k), e4m3(v.float() / v_scale.view(1, hk, 1))
    for lo, hi in ((0, k0), (k1, cap)):                                       # NaN in every slot outside the window
        k8[lo:hi], v8[lo:hi] = 0x7F, 0x7F
    deq, gsz = (lambda b: b.view(F8).double()), hq // hk
    qd = deq(q8).transpose(0, 1)                                              # [hq, rows, 128]
    kd = deq(k8)[k0:k1].repeat_interleave(gsz, dim=1).transpose(0, 1)
    vd = (deq(v8)[k0:k1] * v_scale.view(1, hk, 1).double()).repeat_interleave(gsz, dim=1).transpose(0, 1)
    s = qd @ kd.transpose(1, 2)
    mx = s.max(-1, keepdim=True).values
    p = torch.exp2(s - mx)
    l = p.sum(-1, keepdim=True)
    out64 = ((p @ vd) / l).transpose(0, 1)
    lse64 = (mx + torch.log2(l)).squeeze(-1) * math.log(2)
    p8 = (p * 128).float().to(F8).double()
    emu64 = ((p8 @ vd) / (l * 128)).transpose(0, 1)
    _REFS[case] = (q8, k8, v8, v_scale, out64, lse64, emu64)
    return _REFS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_attention_kv8(ops, case):
    rows, hq, hk, k0, keys, strided, _ = case
    q8, k8, v8, v_scale, out64, lse64, emu64 = _attn_reference(case)
    view = ops.Kv8CacheView(k8.cuda(), v8.cuda(), v_scale.cuda())
    if strided:
        qbuf = torch.full((rows, hq * HD + 48), 0x7F, dtype=torch.uint8, device="cuda")
        obuf = torch.full((rows, hq * HD + 24), 7.0, dtype=BF, device="cuda")
        qg, og = qbuf[:, 16:16 + hq * HD].view(rows, hq, HD), obuf[:, 8:8 + hq * HD].view(rows, hq, HD)
        qg.copy_(q8)
    else:
        qg, og = q8.cuda(), None
    out, lse = ops.attention_kv8(qg, view, k0 + keys, out=og, return_lse=True, kv_start=k0)
    if strided:
        assert bool((obuf[:, :8] == 7.0).all()) and bool((obuf[:, 8 + hq * HD:] == 7.0).all()), "columns outside the output window were written"
    out, lse = out.cpu(), lse.cpu()
    rel, rel_emu = rel_l2(out, out64), rel_l2(emu64, out64)
    lse_err = (lse.double() - lse64).abs().max().item()
    print(f"attention_kv8 {case}: rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}, lse err {lse_err:.2e}")
    assert rel <= 1.25 * rel_emu + 1e-3 and lse_err <= 2e-3          # (NaN compares false)


def _rollout(paging=None, prior=False, **model_kw):
    """The tiny rollout of test_hip_model.py through CausalInferencePipeline: (latents, integer trace, fixture, manager, requests).
    `prior`: another clip (4 x the noise) runs on the same pipeline and caches first."""
    from fixture_io import golden
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.pipeline import CausalInferencePipeline
    from test_hip_model import _pipeline
    fx, cfg = golden("rollout_tiny.npz"), O.tiny_config()
    m, gen, args = _pipeline(cfg, O.init_weights(cfg, seed=0), fx["steps"].tolist(), float(fx["shift"]), **model_kw)
    args.kv_cache_tokens, args.pair_forwards = min(int(fx["cache_tokens"]), 21 * cfg.frame_seqlen), None
    pe = fx["prompt_embeds"].cuda()
    pipe = CausalInferencePipeline(args, "cuda", generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": pe}, vae=None)
    kvm, reqs = KVCacheManager("cuda"), [KVCacheRequest("req0")]
    if paging:
        pipe._initialize_kv_cache(kvm, reqs, BF)
        [kvm.enable_paging(reqs[0], f"layer_{l}", paging) for l in range(cfg.num_layers)]
    for scale in ([4.0] if prior else []) + [1.0]:
        m.index_trace = []
        out = pipe.inference(noise=(fx["noise"].float() * scale).to(BF).cuda(), text_prompts=["x"], kv_cache_manager=kvm, kv_cache_requests=reqs,
                             initial_latent=None, decode_mode=DecodeMode.NO_DECODE, free_cache_before_vae=False,
                             renoise=[fx[f"renoise_{i}"] for i in range(int(fx["num_renoise"]))])
    assert kvm.get_raw(reqs[0], "layer_0").dtype == (torch.uint8 if model_kw.get("kv_cache_dtype") else BF)
    return out.cpu(), m.index_trace, fx, kvm, reqs


def _emulated_oracle_rollout(fx, monkeypatch):
    """The wan_oracle rollout with its self-attention replaced by the fp64 emulation of the 8-bit path: q, K, V and P rounded to e4m3 as
    the contract states, v_scale per layer and head (re)calibrated by an append at slot 0 (keys == rows).  Cross-attention
    (text_len keys) keeps the oracle's own function."""
    cfg, real, scales, calls = O.tiny_config(), O.attention, {}, [0]

    def emulated(q, k, v, impl="sdpa"):
        if k.shape[1] == cfg.text_len:
            return real(q, k, v, impl)
        layer, calls[0] = calls[0] % cfg.num_layers, calls[0] + 1
        if k.shape[1] == q.shape[1]:
            scales[layer] = torch.exp2(torch.ceil(torch.log2(4 * v.float().abs().amax(dim=(0, 1, 3))))).view(1, 1, -1, 1)
        deq = lambda x: e4m3(x).view(F8).double().transpose(1, 2)             # [B, H, L, 128]
        qd, kd, vd = deq(q.float() * Q_SCALE), deq(k), deq(v.float() / scales[layer]) * scales[layer].transpose(1, 2).double()
        s = qd @ kd.transpose(-1, -2)
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        return (((p * 128).float().to(F8).double() @ vd) / (128 * p.sum(-1, keepdim=True))).transpose(1, 2).to(q.dtype).contiguous()
    monkeypatch.setattr(O, "attention", emulated)
    state = O.CacheState.allocate(cfg, 1, BF, cache_tokens=min(int(fx["cache_tokens"]), 21 * cfg.frame_seqlen))
    out, _ = O.inference(O.init_weights(cfg, seed=0), cfg, fx["noise"], list(fx["prompt_embeds"]), fx["steps"].tolist(), shift=float(fx["shift"]),
                         renoise=[fx[f"renoise_{i}"] for i in range(int(fx["num_renoise"]))], num_frame_per_block=3, state=state)
    return out


def test_rollout_kv8(monkeypatch):
    """Integer cache state = the bf16 run's = the reference trace; the latents are as close to the wan_oracle rollout as 1.5 x the
    distance the oracle itself shows with the emulated 8-bit attention; a clip does not depend on what its caches held before; the
    8-bit views live in the manager's per-request store and go with `free`."""
    out8, trace8, fx, kvm, reqs = _rollout(kv_cache_dtype="fp8_e4m3")
    out16, trace16 = _rollout()[:2]
    assert trace8 == trace16 == [tuple(r) for r in fx["trace"].tolist()]
    d8, d_emu = rel_l2(out8, fx["out"]), rel_l2(_emulated_oracle_rollout(fx, monkeypatch), fx["out"])
    print(f"rollout_tiny vs the oracle rollout: fp8_e4m3 cache {d8:.3e}; oracle with emulated 8-bit attention {d_emu:.3e}; bf16 cache "
          f"{rel_l2(out16, fx['out']):.3e}")
    assert d8 <= 1.5 * d_emu
    assert torch.equal(_rollout(prior=True, kv_cache_dtype="fp8_e4m3")[0], out8), "a clip depends on the clip before it"
    assert type(kvm.request_to_kv_caches["req0"].views["layer_0"][1]).__name__ == "Kv8CacheView"
    kvm.free(reqs[0])
    assert "req0" not in kvm.request_to_kv_caches          # ... and with it the views: the model keeps none of its own


def test_refused_combinations():
    from inferix_amd.wan.causal_model import HipCausalWanModel, ParallelConfig
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        HipCausalWanModel(dim=256, num_heads=2, num_layers=1, kv_cache_dtype="int8")
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        HipCausalWanModel(dim=256, num_heads=2, num_layers=1, kv_cache_dtype="fp8_e4m3", parallel_config=ParallelConfig(ulysses_size=2, world_size=2))
    with pytest.raises(NotImplementedError, match="rolling eviction"):
        HipCausalWanModel(dim=256, num_heads=2, num_layers=1, kv_cache_dtype="fp8_e4m3", local_attn_size=3)
    with pytest.raises(NotImplementedError, match="paged caches"):
        _rollout(paging=O.tiny_config().frame_seqlen, kv_cache_dtype="fp8_e4m3")
    cfg, W = O.tiny_config(), O.init_weights(O.tiny_config(), seed=0)
    W["blocks.0.self_attn.norm_k.weight"] = W["blocks.0.self_attn.norm_k.weight"] * 40         # sqrt(2 * 256) * 40 > 448
    from test_hip_model import build
    with pytest.raises(ValueError, match="e4m3 range"):
        build(cfg, W, kv_cache_dtype="fp8_e4m3")
    assert build(cfg, W).kv8 is False and HipCausalWanModel(dim=256, num_heads=2, num_layers=1, kv_cache_dtype="fp8_e4m3").v_direct is False

"""The 8-bit cache's multi-session launches on the GPU: ifx_attn_fwd_kv8_multi and ifx_rmsnorm_rope_kv8_append_multi against the
single launches item by item (bit for bit), one set against fp64 attention over the dequantised bytes, and the two-session serving
scenario of test_hip_serving.py on an fp8_e4m3 config."""
import pytest
import torch

import wan_oracle as O
from test_hip_attn_kv8 import BF, EPS, GRID_HW, HD, RING, _attn_reference, ops  # noqa: F401  (ops: the module fixture)
from util import rel_l2

pytestmark = pytest.mark.gpu
EIGHT = ((1, 0, 1), (33, 0, 63), (256, 0, 64), (300, 0, 65), (33, 0, 200), (300, 0, 200), (33, 70, 200), (256, 0, 1))
#         hq hk strided items (rows, kv_start, keys)
SETS = [(2, 2, False, ((300, 0, 200),)),
        (4, 2, False, ((33, 0, 1), (300, 0, 64 * (RING + 2) + 5))),
        (4, 2, False, EIGHT),
        (2, 2, False, EIGHT),
        (2, 2, False, ((300, 0, 200), (300, 0, 200), (33, 0, 63))),          # equal items: ties in both orderings
        (4, 2, True, ((300, 0, 200), (33, 70, 200)))]


@pytest.mark.parametrize("hq,hk,strided,items", SETS, ids=lambda v: str(v) if isinstance(v, (int, bool)) else f"{len(v)}items")
def test_attention_kv8_multi(ops, hq, hk, strided, items):
    refs = [_attn_reference((rows, hq, hk, k0, keys, False, False)) for rows, k0, keys in items]
    call, bufs = [], []
    for (rows, k0, keys), (q8, k8, v8, v_scale, *_) in zip(items, refs):
        view = ops.Kv8CacheView(k8.cuda(), v8.cuda(), v_scale.cuda())          # 0x7F (NaN) in every slot outside the window
        qbuf = torch.full((rows, hq * HD + 48), 0x7F, dtype=torch.uint8, device="cuda")
        obuf = torch.full((rows, hq * HD + 24), 7.0, dtype=BF, device="cuda")
        qg, og = qbuf[:, 16:16 + hq * HD].view(rows, hq, HD), obuf[:, 8:8 + hq * HD].view(rows, hq, HD)
        if not strided:
            qg, og = torch.empty(rows, hq, HD, dtype=torch.uint8, device="cuda"), torch.full((rows, hq, HD), 7.0, dtype=BF, device="cuda")
        qg.copy_(q8)
        call.append((qg, view, k0 + keys, og, k0))
        bufs.append(obuf)
    ops.attention_kv8_multi(call, hq)
    for i, ((qg, view, k1, og, k0), obuf, ref) in enumerate(zip(call, bufs, refs)):
        alone = ops.attention_kv8(qg, view, k1, kv_start=k0)
        assert torch.equal(og, alone), f"item {i} {items[i]} differs from its single launch"
        if strided:
            assert bool((obuf[:, :8] == 7.0).all()) and bool((obuf[:, 8 + hq * HD:] == 7.0).all()), "columns outside the output window were written"
        if items is EIGHT:          # not resting on the single launch alone: the rule of test_attention_kv8
            out64, emu64 = ref[4], ref[6]
            rel, rel_emu = rel_l2(og.cpu(), out64), rel_l2(emu64, out64)
            print(f"attention_kv8_multi hq {hq} item {items[i]}: rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}")
            assert rel <= 1.25 * rel_emu + 1e-3


#                                       rows local_start start_frame
@pytest.mark.parametrize("heads,items", [(2, ((300, 37, 5),)), (2, ((1, 0, 0), (65, 37, 5), (300, 0, 2))), (16, ((65, 37, 5), (1, 37, 0), (300, 0, 7)))])
def test_append_multi_bytes(ops, heads, items):
    dim, freqs = heads * HD, torch.view_as_real(O.rope_freqs(HD)).contiguous().cuda()
    g = torch.Generator().manual_seed(len(items) + heads)
    wq, wk = ((1 + 0.1 * torch.randn(dim, generator=g)).to(BF).cuda() for _ in range(2))
    qkv_all = (torch.randn(sum(r for r, _, _ in items), 3 * dim + 8, generator=g) * 2).to(BF).cuda()      # rows of one buffer, strided
    got, want, row = [], [], 0
    for i, (rows, start, frame) in enumerate(items):
        rope = ops.RopeGridSpec(freqs, frame, *GRID_HW, q_scale=ops.attn_q_prescale(HD)[0] * (1 + i))
        v_scale = torch.tensor([2.0 ** ((h + i) % 3 - 1) for h in range(heads)]).cuda()
        for dst in (got, want):
            kc, vc = (torch.full((start + rows + 5, heads, HD), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
            q8 = torch.full((rows, dim), 0xA5, dtype=torch.uint8, device="cuda")
            dst.append((qkv_all[row:row + rows, :3 * dim], rope, ops.Kv8CacheView(kc, vc, v_scale), start, q8))
        ops.rmsnorm_rope_kv8_append(want[-1][0], wq, wk, EPS, rope, want[-1][2], start, dim, q_out=want[-1][4])
        row += rows
    ops.rmsnorm_rope_kv8_append_multi(got, wq, wk, EPS, dim)
    for (rows, start, _), g_, w_ in zip(items, got, want):
        assert torch.equal(g_[4], w_[4]) and torch.equal(g_[2].k, w_[2].k) and torch.equal(g_[2].v, w_[2].v), (rows, start)
        for c in (g_[2].k, g_[2].v):
            assert bool((c[:start] == 0xA5).all()) and bool((c[start + rows:] == 0xA5).all()), "bytes outside the appended slots changed"


def test_two_sessions_kv8(tmp_path, monkeypatch, ops):
    """Session b opens two blocks after session a; three joint steps.  Each session's latents equal the session served alone and the
    same scenario with attn_multi = False, bit for bit, and the ragged steps took the multi entry points."""
    import yaml
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.serving import SessionBatch
    cfg = O.tiny_config()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3, independent_first_frame=False,
                context_noise=0, timestep_shift=5.0, kv_cache_tokens=21 * cfg.frame_seqlen, kv_cache_dtype="fp8_e4m3",
                latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim, ffn_dim=cfg.ffn_dim,
                                  freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim, num_heads=cfg.num_heads,
                                  num_layers=cfg.num_layers, eps=cfg.eps))
    (tmp_path / "sf.yaml").write_text(yaml.safe_dump(conf))
    gen = torch.Generator().manual_seed(5)
    embeds = {p: torch.randn(cfg.text_len, cfg.text_dim, generator=gen).to(BF).cuda() for p in ("prompt A", "prompt B")}
    pipe = SelfForcingPipeline(str(tmp_path / "sf.yaml"), vae=None,
                               text_encoder=lambda text_prompts: {"prompt_embeds": torch.stack([embeds[p] for p in text_prompts])})
    torch.save({"generator": {"model." + k: v for k, v in O.init_weights(cfg, seed=0).items()}}, tmp_path / "ckpt.pt")
    pipe.load_checkpoint(str(tmp_path / "ckpt.pt"), use_ema=False)
    pipe.setup_devices(low_memory=False, verbose=False)
    model = pipe.pipeline.generator.model
    assert model.kv8 and model.attn_multi is True
    calls = {"attn": 0, "append": 0}
    for key, name in (("attn", "attention_kv8_multi"), ("append", "rmsnorm_rope_kv8_append_multi")):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _k=key, _f=real, **kw: (calls.__setitem__(_k, calls[_k] + 1), _f(*a, **kw))[1])

    def scenario():
        sb, lat = SessionBatch(pipe, max_sessions=2), {"a": [], "b": []}
        a = sb.open("prompt A", seed=1)
        lat["a"] += [sb.step()[a].clone() for _ in range(2)]
        b = sb.open("prompt B", seed=2)
        for _ in range(3):
            out = sb.step()
            lat["a"].append(out[a].clone()), lat["b"].append(out[b].clone())
        sb.close_all()
        return {k: torch.cat(v, dim=1) for k, v in lat.items()}
    joint, taken = scenario(), dict(calls)
    assert taken["attn"] > 0 and taken["attn"] == taken["append"] and taken["attn"] % cfg.num_layers == 0, taken
    monkeypatch.setattr(model, "attn_multi", False)
    per_sample = scenario()
    assert calls == taken, "attn_multi = False still took the multi entry points"
    for name, prompt, seed, blocks in (("a", "prompt A", 1, 5), ("b", "prompt B", 2, 3)):
        solo = SessionBatch(pipe, max_sessions=1)
        s = solo.open(prompt, seed=seed)
        alone = solo.run(blocks)[s]
        solo.close(s)
        assert torch.isfinite(joint[name].float()).all() and joint[name].shape == alone.shape
        assert torch.equal(joint[name], per_sample[name]), f"session {name}: multi launches differ from per-sample launches"
        assert torch.equal(joint[name], alone), f"session {name}: joint differs from the session served alone"

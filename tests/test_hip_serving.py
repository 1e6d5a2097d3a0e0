"""SessionBatch on the GPU, tiny synthetic model and VAE: two sessions, the second opened after the first has made two steps, three more
steps, then the first closed.  Each session's latents against the same prompt, seed and block count served alone; each session's
streamed frames against the one-shot decode of its own latents (rgb24 and nv12)."""
import pytest
import torch

import vae_oracle as V
import wan_oracle as O
from fixture_io import golden, weights_checksum
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """The tiny configuration of tests/test_hip_streaming_continuous.py, with a text encoder that tells prompts apart."""
    import yaml
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.vae import HipWanVAEWrapper
    g = golden("vae_decode.npz")
    vcfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    VW = V.make_decoder_params(vcfg, int(g["seed"]))
    assert weights_checksum(VW) == int(g["weights_checksum"])
    vae = HipWanVAEWrapper(VW, dim=vcfg.dim)
    cfg = O.tiny_config()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                independent_first_frame=False, context_noise=0, timestep_shift=5.0, kv_cache_tokens=21 * cfg.frame_seqlen,
                latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim,
                                  ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim,
                                  num_heads=cfg.num_heads, num_layers=cfg.num_layers, eps=cfg.eps))
    tmp = tmp_path_factory.mktemp("sessions")
    path = tmp / "sf.yaml"
    path.write_text(yaml.safe_dump(conf))
    gen = torch.Generator().manual_seed(5)
    embeds = {}

    def encoder(text_prompts):
        for p in text_prompts:
            if p not in embeds:
                e = torch.zeros(cfg.text_len, cfg.text_dim)
                n = 4 + len(embeds) * 5
                e[:n] = torch.randn(n, cfg.text_dim, generator=gen)
                embeds[p] = e.to(BF).cuda()
        return {"prompt_embeds": torch.stack([embeds[p] for p in text_prompts])}
    p = SelfForcingPipeline(str(path), text_encoder=encoder, vae=vae)
    ck = tmp / "ckpt.pt"
    torch.save({"generator": {"model." + k: v for k, v in O.init_weights(cfg, seed=0).items()}}, ck)
    p.load_checkpoint(str(ck), use_ema=False)
    p.setup_devices(low_memory=False, verbose=False)
    p.frame_hw = (8 * cfg.latent_h, 8 * cfg.latent_w)
    return p


@pytest.fixture(scope="module")
def served(pipe):
    """The scenario, run once: per session its latents, its stream's frames and what its callback got; the same sessions served alone."""
    from inferix_amd.serving import SessionBatch
    sb = SessionBatch(pipe, max_sessions=2)
    got = {"a": [], "b": []}
    lat = {"a": [], "b": []}
    a = sb.open("prompt A", seed=1, continuous=True, keep_video=True, stream_callback=lambda f: got["a"].append(f.clone()))
    for _ in range(2):
        out = sb.step()
        lat["a"].append(out[a].clone())
    b = sb.open("prompt B", seed=2, continuous=True, keep_video=True, pixel_format="nv12", stream_callback=lambda f: got["b"].append(f.clone()))
    for _ in range(3):
        out = sb.step()
        lat["a"].append(out[a].clone())
        lat["b"].append(out[b].clone())
    sb.close(a)
    video = {"a": a.stream.video(), "b": None}
    assert a.closed and sb.sessions == [b] and (a.block, b.block) == (5, 3)
    sb.close(b)
    video["b"] = b.stream.video()
    assert not sb.kvm.request_to_kv_caches
    alone = {}
    for name, prompt, seed, blocks in (("a", "prompt A", 1, 5), ("b", "prompt B", 2, 3)):
        solo = SessionBatch(pipe, max_sessions=1)
        s = solo.open(prompt, seed=seed)
        alone[name] = solo.run(blocks)[s]
        solo.close(s)
    torch.cuda.synchronize()
    return dict(lat={k: torch.cat(v, dim=1) for k, v in lat.items()}, got=got, video=video, alone=alone)


@pytest.fixture(scope="module")
def yardstick(pipe):
    """The parent's own batching: num_samples = 2 against two num_samples = 1 runs of CausalInferencePipeline.inference with the same
    noise and `renoise` tensors — the largest relative L2 distance between a batch row and its solo run."""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    inner, T = pipe.pipeline, 15
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(2, T, *pipe.latent_shape, generator=g).to(BF).cuda()
    eps = [torch.randn(2, 3, *pipe.latent_shape, generator=g).to(BF).cuda() for _ in range(3 * T // 3)]

    def run(rows, prompts):
        kvm = KVCacheManager(device=pipe.device)
        reqs = [KVCacheRequest(f"y{i}") for i in range(len(prompts))]
        out = inner.inference(noise=noise[rows], text_prompts=prompts, kv_cache_manager=kvm, kv_cache_requests=reqs,
                              decode_mode=DecodeMode.NO_DECODE, renoise=[e[rows].flatten(0, 1) for e in eps])
        for r in reqs:
            if r.request_id in kvm.request_to_kv_caches:
                kvm.free(r)
        return out
    both = run(slice(0, 2), ["prompt A", "prompt B"])
    solo = [run(slice(i, i + 1), [p]) for i, p in enumerate(["prompt A", "prompt B"])]
    torch.cuda.synchronize()
    return max(rel_l2(both[i:i + 1].cpu(), solo[i].cpu()) for i in range(2))


def test_each_sessions_latents_equal_the_session_served_alone(served, yardstick):
    """Within 2 x the yardstick; torch.equal when the yardstick is 0.

    Measured on an MI355X (profiles/r27_sessions.md): yardstick 0, both sessions bit-identical to their solo runs."""
    for name in ("a", "b"):
        lat, alone = served["lat"][name], served["alone"][name]
        assert lat.shape == alone.shape and torch.isfinite(lat.float()).all()
        d = rel_l2(lat.cpu(), alone.cpu())
        print(f"SESSIONS|session {name}: joint vs alone {d:.3e}; yardstick (num_samples 2 vs 1) {yardstick:.3e}")
        if yardstick == 0.0:
            assert torch.equal(lat, alone), (name, d)
        else:
            assert d <= 2 * yardstick, (name, d, yardstick)
    assert not torch.equal(served["lat"]["a"][:, :9], served["lat"]["b"])          # two sessions, two videos


def test_streamed_frames_equal_the_one_shot_decode(pipe, served):
    from inferix_amd import hip_ops as ops
    H, W = pipe.frame_hw
    for name, blocks in (("a", 5), ("b", 3)):
        z = served["lat"][name].permute(0, 2, 1, 3, 4)
        u8 = pipe.pipeline.vae.model.fork().cached_decode_u8(z)
        frames = 1 + 4 * (3 * blocks - 1)
        assert tuple(u8.shape) == (frames, H, W, 3)
        want = u8 if name == "a" else ops.rgb8_to_yuv420(u8, layout="nv12")
        video, cbs = served["video"][name], served["got"][name]
        assert video.dtype == torch.uint8 and not video.is_cuda and video.shape[0] == 1
        assert torch.equal(video[0], want.cpu()), name
        assert [f.shape[0] for f in cbs] == [9] + [12] * (blocks - 1)              # one callback per block of THIS session, in order
        assert torch.equal(torch.cat(cbs, dim=0), want.cpu()), name

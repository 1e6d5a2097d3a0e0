"""`continuous=True` streaming of the few-step Self-Forcing pipeline: one decoder stream for the whole call, uint8 frames
finished on the device — every unique latent frame decoded once, in one seamless stream, bit-identical to the one-shot decode of those
latents.  The tiny configuration of test_hip_vae.py::test_pipeline_takes_the_hip_vae."""
import pytest
import torch

import vae_oracle as V
import wan_oracle as O
from fixture_io import golden, weights_checksum

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SEED = 3
RUN = dict(num_segments=2, segment_length=6, overlap_frames=3)


def finish(pixels: torch.Tensor) -> torch.Tensor:
    """`_to_frames` + `emit` of the per-block callback on `decode_to_pixel` output `[B, T, 3, H, W]` -> uint8 `[B, T, H, W, 3]`."""
    v = (pixels * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2).contiguous()
    return torch.clamp(v * 255.0, 0, 255).to(torch.uint8)


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
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
    tmp = tmp_path_factory.mktemp("sf_continuous")
    path = tmp / "sf.yaml"
    path.write_text(yaml.safe_dump(conf))
    pe = torch.randn(1, cfg.text_len, cfg.text_dim, generator=torch.Generator().manual_seed(5)).to(BF).cuda()
    p = SelfForcingPipeline(str(path), text_encoder=lambda text_prompts: {"prompt_embeds": pe.expand(len(text_prompts), -1, -1)},
                            vae=vae)
    ck = tmp / "ckpt.pt"
    torch.save({"generator": {"model." + k: v for k, v in O.init_weights(cfg, seed=0).items()}}, ck)
    p.load_checkpoint(str(ck), use_ema=False)
    p.setup_devices(low_memory=False, verbose=False)
    p.frame_hw = (8 * cfg.latent_h, 8 * cfg.latent_w)
    return p


@pytest.fixture(scope="module")
def runs(pipe):
    """The same two-segment call under the same seed, three ways; computed once, shared, never written.
      old        without `continuous` (the per-block path as it was), with the segments' latents recorded on the way —
                 the inner pipeline runs with NO_DECODE and the decode draws no random numbers, so these ARE the latents of the seed
      new        with `continuous=True`
      want       the one-shot decode of the unique latents cat(lat0, lat1[:, 3:]), finished by the torch chain."""
    segment = pipe._generate_segment_with_streaming
    lats = []

    def recording(**kw):
        video, lat = segment(**kw)
        lats.append(lat.clone())
        return video, lat
    old_cb, new_cb = [], []
    pipe._generate_segment_with_streaming = recording
    try:
        torch.manual_seed(SEED)
        old = pipe.run_streaming_generation(["p0", "p1"], stream_callback=lambda f: old_cb.append(f.cpu()), **RUN)
    finally:
        del pipe._generate_segment_with_streaming
    torch.manual_seed(SEED)
    new = pipe.run_streaming_generation(["p0", "p1"], stream_callback=lambda f: new_cb.append(f.clone()), continuous=True, **RUN)
    lat0, lat1 = lats
    assert lat0.shape[1] == 6 and lat1.shape[1] == 6 and torch.equal(lat1[:, :3], lat0[:, -3:])
    unique = torch.cat([lat0, lat1[:, 3:]], dim=1)
    want = finish(pipe.pipeline.vae.decode_to_pixel(unique, use_cache=False)).cpu()
    return dict(old=old, old_cb=old_cb, new=new, new_cb=new_cb, want=want, unique=unique)


def test_two_segments_are_one_seamless_stream(pipe, runs):
    H, W = pipe.frame_hw
    new, cbs, want = runs["new"], runs["new_cb"], runs["want"]
    assert pipe.total_frames(**RUN) == 9 and want.shape == (1, 33, H, W, 3)
    assert [tuple(f.shape) for f in cbs] == [(9, H, W, 3), (12, H, W, 3), (12, H, W, 3)]        # the overlap block is not emitted again
    assert all(f.dtype == torch.uint8 and not f.is_cuda for f in cbs)
    assert new.dtype == torch.uint8 and not new.is_cuda and tuple(new.shape) == (1, 33, H, W, 3)
    assert torch.equal(new, want)
    assert torch.equal(torch.cat(cbs, dim=0), want[0])


def test_existing_mode_is_unchanged(pipe, runs):
    """Without the keyword: float frames in [0, 1], 9 per generated block (every block restarts the decoder, as upstream) — three
    generated blocks in the two segments (the block callback never sees the overlap prefill, in either mode), so 27 frames where the
    continuous stream has 33 — and each block equal to the per-block decode it has always been."""
    H, W = pipe.frame_hw
    old, cbs, unique = runs["old"], runs["old_cb"], runs["unique"]
    assert old.dtype == torch.float32 and not old.is_cuda and tuple(old.shape) == (1, 27, H, W, 3)
    assert len(cbs) == 3 and all(f.dtype == torch.uint8 and tuple(f.shape) == (9, H, W, 3) for f in cbs)
    for k in range(3):
        blk = pipe.pipeline.vae.decode_to_pixel(unique[:, 3 * k:3 * k + 3], use_cache=True, chunk_size=1)
        blk = (blk * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2)
        assert torch.equal(old[:, 9 * k:9 * k + 9], blk.cpu()), k
        assert torch.equal(cbs[k], torch.clamp(blk[0] * 255.0, 0, 255).to(torch.uint8).cpu()), k


def test_keep_video_false_returns_none_and_still_streams(pipe, runs):
    got = []
    torch.manual_seed(SEED)
    out = pipe.run_streaming_generation(["p0", "p1"], stream_callback=lambda f: got.append(f.clone()), continuous=True,
                                        keep_video=False, **RUN)
    assert out is None
    assert [f.shape[0] for f in got] == [9, 12, 12] and torch.equal(torch.cat(got), runs["want"][0])


def test_interactive_stop_delivers_what_was_generated(pipe, runs):
    """A STOP that is waiting at the boundary in front of segment 1: the loop ends there, and every frame of segment 0 has reached the
    callback by the time the call returns (the stream is flushed on the way out)."""
    from inferix_amd.core import ControlCommand, InteractiveSession, SessionState
    session = InteractiveSession()
    segment = pipe._generate_segment_with_streaming
    calls = []

    def then_stop(**kw):
        out = segment(**kw)
        calls.append(kw.get("frame_stream"))
        session.submit_input(control=ControlCommand.STOP)
        return out
    got = []
    pipe._generate_segment_with_streaming = then_stop
    try:
        torch.manual_seed(SEED)
        out = pipe.run_interactive_generation(session, "p0", stream_callback=lambda f: got.append(f.clone()), continuous=True, **RUN)
    finally:
        del pipe._generate_segment_with_streaming
    assert len(calls) == 1 and calls[0] is not None and session.state != SessionState.ERROR
    assert [f.shape[0] for f in got] == [9, 12]
    assert torch.equal(torch.cat(got), runs["want"][0, :21])
    assert out.dtype == torch.uint8 and torch.equal(out, runs["want"][:, :21])


def test_refusals(pipe, monkeypatch):
    from inferix_amd.core.types import StreamingMode
    with pytest.raises(ValueError, match="continuous"):
        pipe.run_streaming_generation(["p"], num_segments=1, segment_length=6, continuous=True,
                                      streaming_mode=StreamingMode.DEFERRED_DECODE)
    with pytest.raises(ValueError, match="continuous"):
        pipe._generate_segment_with_streaming("p", None, None, segment_length=6, continuous=True,
                                              streaming_mode=StreamingMode.DEFERRED_DECODE)

    class UpstreamVae:                                   # anything that is not this build's decoder
        model = torch.nn.Identity()

        def decode_to_pixel(self, *a, **k):
            raise AssertionError("not reached")
    monkeypatch.setattr(pipe.pipeline, "vae", UpstreamVae())
    with pytest.raises(ValueError, match="continuous streaming needs the HIP decoder"):
        pipe.run_streaming_generation(["p"], num_segments=1, segment_length=6, continuous=True)


def test_segment_with_its_own_stream_returns_its_frames(pipe, runs):
    """`_generate_segment_with_streaming(continuous=True)` without a `frame_stream`: the segment opens one, flushes it and returns the
    uint8 frames of the segment."""
    torch.manual_seed(SEED)
    video, lat = pipe._generate_segment_with_streaming("p0", None, None, segment_length=6, continuous=True)
    assert lat.shape[1] == 6 and video.dtype == torch.uint8 and torch.equal(video, runs["want"][:, :21])

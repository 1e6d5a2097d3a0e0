"""GPU: `MagiFrameStream` and `MagiPipeline.run_streaming_generation(..., continuous=True)` on the tiny ViT-VAE and the stub DiT of
tests/test_hip_magi_walk.py.  No reference streams MAGI: the yardstick is this build's own non-streaming path (`post_chunk_process`,
`run_text_to_video`, `generate_per_chunk` by hand), which streaming must reproduce bit for bit, frame for frame and in order."""
from types import SimpleNamespace

import pytest
import torch

from test_hip_magi_walk import H_LAT, W_LAT, _count_syncs, _Embedder, _stub_model, _tiny_vae

pytestmark = pytest.mark.gpu
HP, WP = 8 * H_LAT, 8 * W_LAT


def _parts(num_frames=16):
    """(pipeline, config, dit, vae) of test_magi_pipeline_frames_equal_the_per_chunk_decode: chunks of 2 latent frames = 8 video frames,
    `num_frames // 4` latent frames per request."""
    from inferix_amd.pipeline.magi import MagiPipeline
    vae, vcfg = _tiny_vae()
    dit = _stub_model(1, in_channels=vcfg.z_chans)
    rc = dit.runtime_config
    rc.num_steps, rc.window_size, rc.chunk_width, rc.num_frames, rc.temporal_downsample_factor = 8, 4, 2, num_frames, 4
    rc.video_size_h, rc.video_size_w, rc.fps, rc.scale_factor = HP, WP, 16, 0.5
    config = SimpleNamespace(model_config=dit.model_config, engine_config=dit.engine_config, runtime_config=rc)
    return MagiPipeline(config, dit=dit, vae=vae, embedder=_Embedder()), config, dit, vae


def _chunks(config, dit, prefix=None, prompt="a prompt"):
    from inferix_amd.magi.prompt import get_txt_embeddings
    from inferix_amd.magi.schedule import generate_per_chunk
    cap, cap_mask = get_txt_embeddings(prompt, config, _Embedder())
    return [c.clone() for c in generate_per_chunk(dit, prefix, cap, cap_mask)]


def _hwc(config, vae, chunks):
    """`post_chunk_process` of every chunk, permuted to channel-last, on the host: `[T, H, W, 3]`."""
    from inferix_amd.magi.vae import post_chunk_process
    return torch.cat([post_chunk_process(c, config, vae) for c in chunks], dim=0).permute(0, 2, 3, 1).contiguous().cpu()


@pytest.mark.parametrize("slots", [1, 3])
def test_stream_delivers_the_frames_of_post_chunk_process_in_order(slots):
    from inferix_amd.streaming import MagiFrameStream
    _, config, dit, vae = _parts(num_frames=24)
    torch.manual_seed(11)
    chunks = _chunks(config, dit)
    assert len(chunks) == 3
    want = _hwc(config, vae, chunks)
    views, copies = [], []

    def callback(frames):
        assert frames.dtype == torch.uint8 and not frames.is_cuda and tuple(frames.shape) == (8, HP, WP, 3)
        views.append(frames)
        copies.append(frames.clone())
    fs = MagiFrameStream(vae, config, slots=slots, callback=callback, keep=True)
    for c in chunks:
        fs.push(c)
        assert len(fs._inflight) <= slots
    assert fs.frames_pushed == 24
    fs.flush()
    assert len(copies) == 3 and not fs._inflight
    assert torch.equal(torch.cat(copies), want), "the delivered frames differ from post_chunk_process's"
    if slots == 3:                                         # a view outlives `slots - 1` further pushes
        assert torch.equal(views[0], want[:8]) and torch.equal(views[2], want[16:])
        assert len({v.data_ptr() for v in views}) == 3
    video = fs.video()
    assert video.dtype == torch.uint8 and tuple(video.shape) == (1, 24, HP, WP, 3) and torch.equal(video[0], want)
    fs.reset()
    assert fs.video() is None and fs.frames_pushed == 0
    assert want.float().std() > 1.0, "the decoded clip is flat"


def test_stream_needs_the_hip_vae():
    from inferix_amd.pipeline.magi import MagiPipeline
    from inferix_amd.streaming import MagiFrameStream
    _, config, dit, vae = _parts()
    with pytest.raises(TypeError, match="continuous streaming needs the HIP decoder"):
        MagiFrameStream(object(), config)
    with pytest.raises(ValueError, match="slots"):
        MagiFrameStream(vae, config, slots=0)
    pipe = MagiPipeline(config, dit=dit, vae=object(), embedder=_Embedder())
    with pytest.raises(ValueError, match="continuous=True: continuous streaming needs the HIP decoder"):
        pipe.run_streaming_generation(["p"], num_segments=1, continuous=True)
    with pytest.raises(NotImplementedError, match="Streaming generation is not yet implemented"):
        pipe.run_streaming_generation(["p"], num_segments=1)


@pytest.mark.parametrize("image", [False, True])
def test_one_streamed_segment_equals_the_unstreamed_request(image):
    import magi_vit_encoder_util as E
    pipe, config, dit, vae = _parts()
    extra = {"image": E.make_pixels(63, (1, HP, WP, 3)).cuda()} if image else {}
    torch.manual_seed(5)
    want = pipe.run_image_to_video("a prompt", **extra) if image else pipe.run_text_to_video("a prompt")
    n_chunks = 3 if image else 2
    assert tuple(want.shape) == (n_chunks * 8, 3, HP, WP)
    got = []
    torch.manual_seed(5)
    video = pipe.run_streaming_generation(["a prompt"], lambda f: got.append(f.clone()), num_segments=1, continuous=True, **extra)
    assert len(got) == n_chunks, "one callback per chunk"
    assert video.dtype == torch.uint8 and not video.is_cuda and tuple(video.shape) == (1, n_chunks * 8, HP, WP, 3)
    assert torch.equal(video[0], want.permute(0, 2, 3, 1).cpu()) and torch.equal(torch.cat(got), video[0])
    torch.manual_seed(5)
    assert pipe.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True, keep_video=False, **extra) is None


def test_two_segments_the_prefix_ends_inside_a_chunk():
    """`overlap_frames=3` at `chunk_width=2`: segment 2 starts behind a prefix of a chunk and a frame, so its first hand-out is the one
    frame the prefix leaves of chunk 1 (a single latent frame: a single video frame), then two whole chunks."""
    pipe, config, dit, vae = _parts()
    torch.manual_seed(7)
    first = _chunks(config, dit, prompt="one")
    final = torch.cat(first, dim=2)
    assert tuple(final.shape[:3]) == (1, dit.model_config.in_channels, 4)
    second = _chunks(config, dit, prefix=final[:, :, -3:].contiguous(), prompt="two!")
    assert [c.shape[2] for c in first] == [2, 2] and [c.shape[2] for c in second] == [1, 2, 2]
    want = torch.cat([_hwc(config, vae, first), _hwc(config, vae, second)])
    assert want.shape[0] == 16 + 1 + 16
    got = []
    torch.manual_seed(7)
    video = pipe.run_streaming_generation(["one", "two!"], lambda f: got.append(f.clone()), num_segments=2, overlap_frames=3,
                                          continuous=True)
    assert [g.shape[0] for g in got] == [8, 8, 1, 8, 8], "the hand-outs of two segments, the prefix frames never again"
    assert tuple(video.shape) == (1, 33, HP, WP, 3) and torch.equal(video[0], want), "every frame once, segment 2 as by hand"
    assert torch.equal(torch.cat(got), want)


def test_interactive_generation_streams_the_same_frames():
    from inferix_amd.core.interactive import InteractiveSession
    pipe, config, dit, vae = _parts()
    torch.manual_seed(7)
    want = pipe.run_streaming_generation(["one"], None, num_segments=2, overlap_frames=3, continuous=True)
    torch.manual_seed(7)
    got = pipe.run_interactive_generation(InteractiveSession(), "one", num_segments=2, overlap_frames=3, continuous=True)
    assert torch.equal(got, want)


def test_a_streamed_clip_does_not_wait_for_the_device(monkeypatch):
    """With as many slots as chunks, no synchronising call between the first and the last forward of a streamed clip: the property
    test_walk_does_not_wait_for_the_device holds for `walk` alone, with the pushes in between.  Counted: the tensor reads and blocking
    uploads of `_count_syncs`, and every `synchronize` of an event, a stream or the device."""
    from inferix_amd.streaming import MagiFrameStream
    pipe, config, dit, vae = _parts(num_frames=24)
    torch.manual_seed(5)
    pipe.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True)         # plans, tables and arenas exist
    counted = []
    _count_syncs(monkeypatch, counted)
    for owner, name in ((torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize")):
        orig = getattr(owner, name)

        def wrapped(*a, _orig=orig, _name=f"{getattr(owner, '__name__', 'cuda')}.{name}", **k):
            counted.append(_name)
            return _orig(*a, **k)
        monkeypatch.setattr(owner, name, wrapped)
    seen = []
    forward = dit.forward

    def stamped(*a, **k):
        if not seen:
            counted.clear()
        seen.append(list(counted))
        return forward(*a, **k)
    dit.forward = stamped
    delivered = []
    fs = MagiFrameStream(vae, config, slots=3, callback=delivered.append, keep=False)
    torch.manual_seed(5)
    pipe.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True, frame_stream=fs)
    assert len(delivered) == 3 and fs.frames_pushed == 24
    # 3 chunks of 8 steps in a window of 4: chunks 0 and 1 are pushed with forwards still to come
    assert len(seen) > 8 and seen[-1] == [], f"waits between the first and the last forward: {seen[-1]}"


def test_flush_hands_the_vae_back():
    pipe, config, dit, vae = _parts()
    torch.manual_seed(5)
    before = pipe.run_text_to_video("a prompt").clone()
    torch.manual_seed(5)
    video = pipe.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True)
    torch.manual_seed(5)
    after = pipe.run_text_to_video("a prompt")
    assert torch.equal(after, before) and torch.equal(video[0], before.permute(0, 2, 3, 1).cpu())


def test_an_exception_in_the_callback_surfaces_and_the_stream_stays_consistent():
    from inferix_amd.streaming import MagiFrameStream
    pipe, config, dit, vae = _parts(num_frames=24)
    calls = []

    def callback(frames):
        calls.append(frames.shape[0])
        if len(calls) == 1:
            raise RuntimeError("the consumer failed")
    fs = MagiFrameStream(vae, config, callback=callback)
    with pytest.raises(RuntimeError, match="the consumer failed"):
        pipe.run_streaming_generation(["a prompt"], callback, num_segments=1, continuous=True, frame_stream=fs)
    fs.flush()                                             # whatever the failed delivery left in flight
    assert not fs._inflight and calls == [8] * (fs.frames_pushed // 8) and 1 <= len(calls) <= 3


def test_the_device_error_word_stops_delivery(monkeypatch):
    """`hip_ops.check_device` patched to raise on its second call (no fault is provoked): the first chunk is delivered, the second and
    everything after it are not, and the error surfaces from the call."""
    from inferix_amd import _hip, hip_ops
    from inferix_amd.streaming import MagiFrameStream
    pipe, config, dit, vae = _parts(num_frames=24)
    check, calls, got = hip_ops.check_device, [], []

    def second_raises(what="", sync=False):
        calls.append(what)
        if len(calls) >= 2:
            raise _hip.HipKernelError(f"{what}: a device-side wait gave up")
        return check(what, sync)
    monkeypatch.setattr(hip_ops, "check_device", second_raises)
    fs = MagiFrameStream(vae, config, callback=got.append)
    with pytest.raises(_hip.HipKernelError, match="MagiFrameStream"):
        pipe.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True, frame_stream=fs)
    assert len(got) == 1 and len(calls) == 2 and not fs._inflight
    fs.flush()
    assert len(got) == 1

"""GPU: YUV 4:2:0 through the decoder, the two frame streams and the two pipelines (`pixel_format="yuv420p"` / `"nv12"`), on the tiny
fixtures of tests/test_hip_frame_stream.py, tests/test_hip_streaming_continuous.py and tests/test_hip_magi_stream.py.  The yardstick is
always the `rgb24` path of the same build, whose bytes go through the integer restatement of tests/yuv_util.py."""
import pytest
import torch

import yuv_util as Y
from test_hip_frame_stream import cuts, tiny  # noqa: F401  (`tiny` is a fixture)
from test_hip_magi_stream import HP, WP, _chunks, _hwc, _parts
from test_hip_streaming_continuous import RUN, SEED, pipe  # noqa: F401  (`pipe` is a fixture)

pytestmark = pytest.mark.gpu
FORMATS = ["yuv420p", "nv12"]


def _bytes(fs):
    """(device bytes, pinned bytes) the stream's slots hold."""
    assert all(s.host is None or s.host.is_pinned() for s in fs._slots)
    return (sum(s.dev.numel() for s in fs._slots if s.dev is not None), sum(s.host.numel() for s in fs._slots if s.host is not None))


# ---- the decoder -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoded(tiny):
    """`cached_decode_u8` of the whole latent in one call on a fork of the decoder: uint8 `[33, 64, 96, 3]` on the host."""
    vae, lat, want, _, _ = tiny
    u8 = vae.model.fork().cached_decode_u8(lat.permute(0, 2, 1, 3, 4)).cpu()
    assert torch.equal(u8, want[0])
    return u8


@pytest.mark.parametrize("sizes", [(3,), (1, 2, 3), (2,)], ids=["3,3,..", "1,2,3,..", "2,2,.."])
def test_cached_decode_yuv420_is_the_restatement_of_cached_decode_u8(tiny, decoded, sizes):
    vae, lat, _, _, _ = tiny
    z = lat.permute(0, 2, 1, 3, 4)
    dec = vae.model.fork()
    got = torch.cat([dec.cached_decode_yuv420(z[:, :, a:b]) for a, b in cuts(lat.shape[1], sizes)])
    T, H, W, _ = decoded.shape
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (T, H * 3 // 2, W)
    assert torch.equal(got.cpu(), Y.rgb_to_yuv420(decoded, "i420"))
    if sizes == (3,):                                      # the keywords and a caller's buffer
        dec = vae.model.fork()
        out = torch.empty(9, H * 3 // 2, W, dtype=torch.uint8, device="cuda")
        assert dec.cached_decode_yuv420(z[:, :, :3], out=out, layout="nv12", matrix="bt709", full_range=True) is out
        assert torch.equal(out.cpu(), Y.rgb_to_yuv420(decoded[:9], "nv12", "bt709", True))


# ---- FrameStream -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_stream(tiny):
    """The `rgb24` stream of the same pushes, per slot count: (frames per callback, (device, pinned) bytes)."""
    from inferix_amd.streaming import FrameStream
    vae, lat, want, _, _ = tiny
    out = {}
    for slots in (1, 3):
        got = []
        fs = FrameStream(vae, slots=slots, callback=lambda f: got.append(f.clone()))
        for a, b in cuts(lat.shape[1], (3,)):
            fs.push(lat[:, a:b])
        fs.flush()
        assert torch.equal(torch.cat(got), want[0])
        out[slots] = (got, _bytes(fs))
    return out


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_stream_delivers_the_restatement_of_the_rgb24_stream(tiny, rgb_stream, fmt, slots):
    """`slots=1` is the back-pressure case: every push but the first waits for the block before it."""
    from inferix_amd.streaming import FrameStream
    vae, lat, _, _, _ = tiny
    rgb, rgb_bytes = rgb_stream[slots]
    got = []
    fs = FrameStream(vae, slots=slots, callback=lambda f: got.append(f.clone()), keep=True, pixel_format=fmt)
    for a, b in cuts(lat.shape[1], (3,)):
        fs.push(lat[:, a:b])
        assert len(fs._inflight) <= slots
    fs.flush()
    assert len(got) == len(rgb) == 3 and fs.frames_pushed == 33
    for k, (f, r) in enumerate(zip(got, rgb)):
        T, H, W, _ = r.shape
        assert f.dtype == torch.uint8 and not f.is_cuda and tuple(f.shape) == (T, H * 3 // 2, W), k
        assert torch.equal(f, Y.rgb_to_yuv420(r, fmt)), k
    dev, host = _bytes(fs)
    assert (2 * dev, 2 * host) == rgb_bytes, "1.5 bytes per pixel against 3, device and pinned"
    video = fs.video()
    assert tuple(video.shape) == (1, 33, 64 * 3 // 2, 96) and torch.equal(video[0], torch.cat(got))


def test_frame_stream_matrix_keywords_two_samples_and_refusals(tiny):
    from inferix_amd.streaming import FrameStream
    vae, lat, want, lat2, want2 = tiny
    fs = FrameStream(vae, num_samples=2, keep=True, pixel_format="nv12", matrix="bt709", full_range=True)
    both = torch.cat([lat, lat2], dim=0)
    for a, b in cuts(lat.shape[1], (3,)):
        fs.push(both[:, a:b])
    video = fs.video()
    assert torch.equal(video[0], Y.rgb_to_yuv420(want[0], "nv12", "bt709", True))
    assert torch.equal(video[1], Y.rgb_to_yuv420(want2[0], "nv12", "bt709", True))
    with pytest.raises(ValueError, match="pixel_format is one of"):
        FrameStream(vae, pixel_format="yuv444p")
    with pytest.raises(ValueError, match="matrix is one of"):
        FrameStream(vae, pixel_format="nv12", matrix="bt2020")


def test_device_error_word_stops_delivery_of_yuv_frames(tiny, monkeypatch):
    """As for `rgb24`: `hip_ops.check_device` patched to raise (no fault is provoked); nothing further is delivered."""
    from inferix_amd import _hip, hip_ops
    from inferix_amd.streaming import FrameStream
    vae, lat, _, _, _ = tiny
    got = []
    fs = FrameStream(vae, slots=3, callback=got.append, pixel_format="yuv420p")
    fs.push(lat[:, :1])
    fs.flush()
    assert len(got) == 1

    def raised(what="", sync=False):
        raise _hip.HipKernelError(f"{what}: a device-side wait gave up")
    monkeypatch.setattr(hip_ops, "check_device", raised)
    with pytest.raises(_hip.HipKernelError):
        fs.push(lat[:, 1:2])
        fs.push(lat[:, 2:3])
        fs.flush()
    assert len(got) == 1 and not fs._inflight
    fs.flush()
    assert len(got) == 1


# ---- MagiFrameStream ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def magi():
    """(config, vae, chunks, the `rgb24` frames `[24, H, W, 3]` of `post_chunk_process`, the `rgb24` stream's (device, pinned) bytes per
    slot count)."""
    from inferix_amd.streaming import MagiFrameStream
    _, config, dit, vae = _parts(num_frames=24)
    torch.manual_seed(11)
    chunks = _chunks(config, dit)
    want = _hwc(config, vae, chunks)
    sizes = {}
    for slots in (1, 3):
        fs = MagiFrameStream(vae, config, slots=slots, keep=True)
        for c in chunks:
            fs.push(c)
        assert torch.equal(fs.video()[0], want)
        sizes[slots] = _bytes(fs)
    return config, vae, chunks, want, sizes


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_magi_stream_delivers_the_restatement_of_the_rgb24_frames(magi, fmt, slots):
    from inferix_amd.streaming import MagiFrameStream
    config, vae, chunks, want, sizes = magi
    got = []
    fs = MagiFrameStream(vae, config, slots=slots, callback=lambda f: got.append(f.clone()), keep=True, pixel_format=fmt)
    for c in chunks:
        fs.push(c)
        assert len(fs._inflight) <= slots
    fs.flush()
    assert len(got) == 3 and all(tuple(f.shape) == (8, HP * 3 // 2, WP) and f.dtype == torch.uint8 and not f.is_cuda for f in got)
    assert torch.equal(torch.cat(got), Y.rgb_to_yuv420(want, fmt))
    dev, host = _bytes(fs)
    assert (2 * dev, 2 * host) == sizes[slots]
    assert len(fs._rgb) == 1 and next(iter(fs._rgb.values())).numel() == 8 * HP * WP * 3, "one rgb24 scratch per chunk shape"
    video = fs.video()
    assert tuple(video.shape) == (1, 24, HP * 3 // 2, WP) and torch.equal(video[0], torch.cat(got))
    # after flush() the same vae decodes rgb24 on the current stream to the bytes it gave before
    assert torch.equal(_hwc(config, vae, chunks), want)
    fs.reset()
    assert not fs._rgb and fs.video() is None, "reset() drops the scratch with the kept copies"


# ---- the pipelines -----------------------------------------------------------------------------------------------------------------
def test_self_forcing_pipeline_streams_yuv420p(pipe):
    H, W = pipe.frame_hw
    torch.manual_seed(SEED)
    rgb = pipe.run_streaming_generation(["p0", "p1"], continuous=True, **RUN)
    got = []
    torch.manual_seed(SEED)
    yuv = pipe.run_streaming_generation(["p0", "p1"], stream_callback=lambda f: got.append(f.clone()), continuous=True,
                                        pixel_format="yuv420p", **RUN)
    assert tuple(rgb.shape) == (1, 33, H, W, 3) and tuple(yuv.shape) == (1, 33, H * 3 // 2, W) and yuv.dtype == torch.uint8
    assert torch.equal(yuv, Y.rgb_to_yuv420(rgb, "yuv420p")) and torch.equal(torch.cat(got), yuv[0])
    assert [f.shape[0] for f in got] == [9, 12, 12]
    torch.manual_seed(SEED)
    nv12 = pipe.run_streaming_generation(["p0", "p1"], continuous=True, pixel_format="nv12", color_matrix="bt709", full_range=True, **RUN)
    assert torch.equal(nv12, Y.rgb_to_yuv420(rgb, "nv12", "bt709", True))
    with pytest.raises(ValueError, match="pixel_format 'yuv420p' needs continuous=True"):
        pipe.run_streaming_generation(["p0"], num_segments=1, segment_length=6, pixel_format="yuv420p")
    with pytest.raises(ValueError, match="pixel_format 'nv12' needs continuous=True"):
        pipe._generate_segment_with_streaming("p0", None, None, segment_length=6, pixel_format="nv12")
    own = pipe._make_frame_stream(None, pixel_format="yuv420p", matrix="bt709")
    assert (own.pixel_format, own.matrix, own.full_range) == ("yuv420p", "bt709", False)
    with pytest.raises(ValueError, match="pixel_format='nv12' disagrees with the given frame_stream"):
        pipe.run_streaming_generation(["p0"], continuous=True, frame_stream=own, pixel_format="nv12", **RUN)
    with pytest.raises(ValueError, match="matrix='bt601' disagrees"):
        pipe._generate_segment_with_streaming("p0", None, None, segment_length=6, continuous=True, frame_stream=own, color_matrix="bt601")
    assert own.frames_pushed == 0


def test_magi_pipeline_streams_yuv420p():
    from inferix_amd.core.interactive import InteractiveSession
    mp, config, dit, vae = _parts()
    torch.manual_seed(5)
    rgb = mp.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True)
    got = []
    torch.manual_seed(5)
    yuv = mp.run_streaming_generation(["a prompt"], lambda f: got.append(f.clone()), num_segments=1, continuous=True,
                                      pixel_format="yuv420p")
    assert tuple(rgb.shape) == (1, 16, HP, WP, 3) and tuple(yuv.shape) == (1, 16, HP * 3 // 2, WP)
    assert torch.equal(yuv, Y.rgb_to_yuv420(rgb, "yuv420p")) and torch.equal(torch.cat(got), yuv[0]) and len(got) == 2
    torch.manual_seed(5)
    nv12 = mp.run_interactive_generation(InteractiveSession(), "a prompt", num_segments=1, continuous=True, pixel_format="nv12",
                                         color_matrix="bt709")
    assert torch.equal(nv12, Y.rgb_to_yuv420(rgb, "nv12", "bt709"))
    with pytest.raises(ValueError, match="pixel_format 'yuv420p' needs continuous=True"):
        mp.run_streaming_generation(["a prompt"], None, num_segments=1, pixel_format="yuv420p")


def test_the_device_error_word_stops_a_magi_yuv_stream(monkeypatch):
    """`hip_ops.check_device` patched to raise on its second call (no fault is provoked): one chunk is delivered, no more."""
    from inferix_amd import _hip, hip_ops
    from inferix_amd.streaming import MagiFrameStream
    mp, config, dit, vae = _parts(num_frames=24)
    check, calls, got = hip_ops.check_device, [], []

    def second_raises(what="", sync=False):
        calls.append(what)
        if len(calls) >= 2:
            raise _hip.HipKernelError(f"{what}: a device-side wait gave up")
        return check(what, sync)
    monkeypatch.setattr(hip_ops, "check_device", second_raises)
    fs = MagiFrameStream(vae, config, callback=got.append, pixel_format="yuv420p")
    with pytest.raises(_hip.HipKernelError, match="MagiFrameStream"):
        mp.run_streaming_generation(["a prompt"], None, num_segments=1, continuous=True, frame_stream=fs)
    assert len(got) == 1 and tuple(got[0].shape) == (8, HP * 3 // 2, WP) and len(calls) == 2 and not fs._inflight
    fs.flush()
    assert len(got) == 1

"""`FrameStream` (inferix_amd/streaming.py) on the tiny decoder and latent of tests/golden/vae_decode.npz: a decoder stream that is never
reset, ending in uint8 on the device, equals the one-shot decode of the same latents finished by the torch chain — bit for bit, however
the latent is cut into blocks."""
import pytest
import torch

import vae_oracle as V
from fixture_io import golden, weights_checksum

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def finish(pixels: torch.Tensor) -> torch.Tensor:
    """`_to_frames` + `emit` of the per-block callback on `decode_to_pixel` output `[B, T, 3, H, W]` -> uint8 `[B, T, H, W, 3]`."""
    v = (pixels * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2).contiguous()
    return torch.clamp(v * 255.0, 0, 255).to(torch.uint8)


@pytest.fixture(scope="module")
def tiny():
    g = golden("vae_decode.npz")
    cfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    W = V.make_decoder_params(cfg, int(g["seed"]))
    assert weights_checksum(W) == int(g["weights_checksum"])
    from inferix_amd.vae import HipWanVAEWrapper
    vae = HipWanVAEWrapper(W, dim=cfg.dim)
    lat = g["latent"].cuda()                                       # [1, 3, 16, 8, 12]
    # the golden latent is one block; six more frames of the same kind behind it, so that the chunkings below have boundaries to differ in
    extra = torch.randn(1, 9 - lat.shape[1], *lat.shape[2:], generator=torch.Generator().manual_seed(2)).to(lat)
    lat = torch.cat([lat, extra], dim=1)
    want = finish(vae.decode_to_pixel(lat, use_cache=False)).cpu()         # computed once, shared, never written
    lat2 = torch.randn(lat.shape, generator=torch.Generator().manual_seed(7)).to(lat)
    want2 = finish(vae.decode_to_pixel(lat2, use_cache=False)).cpu()
    return vae, lat, want, lat2, want2


def cuts(T, sizes):
    """Block boundaries: `sizes` cycled until the `T` latent frames are used up."""
    out, i, k = [], 0, 0
    while i < T:
        n = min(sizes[k % len(sizes)], T - i)
        out.append((i, i + n))
        i, k = i + n, k + 1
    return out


@pytest.mark.parametrize("sizes", [(3,), (1, 2, 3), (2,)], ids=["3,3,..", "1,2,3,..", "2,2,.."])
def test_any_chunking_gives_the_one_shot_bytes(tiny, sizes):
    from inferix_amd.streaming import FrameStream
    vae, lat, want, _, _ = tiny
    T = lat.shape[1]
    got = []
    fs = FrameStream(vae, callback=lambda f: got.append(f.clone()), keep=True)
    blocks = cuts(T, sizes)
    for a, b in blocks:
        fs.push(lat[:, a:b])
    fs.flush()
    assert [f.shape[0] for f in got] == [4 * (b - a) - (3 if a == 0 else 0) for a, b in blocks]
    assert all(f.dtype == torch.uint8 and not f.is_cuda and f.shape[1:] == want.shape[2:] for f in got)
    frames = torch.cat(got, dim=0)
    assert frames.shape[0] == 1 + 4 * (T - 1)
    assert torch.equal(frames, want[0])
    video = fs.video()
    assert video.dtype == torch.uint8 and not video.is_pinned() and torch.equal(video, want)


def test_parent_decoder_does_not_disturb_a_fork(tiny):
    """`clear_cache()` and a whole `decode_to_pixel` on the parent between two pushes (what `_cleanup_segment_memory` and any other
    user of the VAE do): the stream goes on as if nothing had happened, and shares the parent's packed weights."""
    from inferix_amd.streaming import FrameStream
    vae, lat, want, lat2, want2 = tiny
    fs = FrameStream(vae, keep=True)
    dec = fs._decoders[0]
    assert dec is not vae.model and dec.W is vae.model.W and dec._rings is not vae.model._rings and dec._scratch is not vae.model._scratch
    fs.push(lat[:, :3])
    vae.model.clear_cache()
    other = finish(vae.decode_to_pixel(lat2, use_cache=True, chunk_size=1)).cpu()
    vae.model.clear_cache()
    fs.push(lat[:, 3:])
    assert torch.equal(fs.video(), want)
    assert torch.equal(other, want2)                               # nor does the stream disturb the parent


def test_two_samples_each_equal_their_own_decode(tiny):
    from inferix_amd.streaming import FrameStream
    vae, lat, want, lat2, want2 = tiny
    order = []
    fs = FrameStream(vae, num_samples=2, callback=lambda f: order.append(f.clone()), keep=True)
    both = torch.cat([lat, lat2], dim=0)
    for a, b in cuts(lat.shape[1], (3,)):
        fs.push(both[:, a:b])
    video = fs.video()
    assert video.shape == (2,) + tuple(want.shape[1:])
    assert torch.equal(video[0], want[0]) and torch.equal(video[1], want2[0])
    # delivery is block by block, sample by sample
    assert torch.equal(torch.cat(order[0::2]), want[0]) and torch.equal(torch.cat(order[1::2]), want2[0])


def test_back_pressure_keeps_order_and_bytes(tiny):
    """Two slots, five blocks: the third push finds both buffers in flight and has to wait for the oldest.  Delivery stays in push
    order with the right bytes, no more than `slots` blocks are ever in flight, and a view is still intact `slots - 1` pushes later."""
    from inferix_amd.streaming import FrameStream
    vae, lat, want, _, _ = tiny
    T = lat.shape[1]
    blocks = cuts(T, (1, 1, 1, 1, T))                              # five blocks: four of one latent frame, the rest in the fifth
    assert len(blocks) == 5
    seen, views = [], []

    def cb(f):
        seen.append(f.clone())
        views.append(f)
    fs = FrameStream(vae, slots=2, callback=cb)
    for a, b in blocks:
        fs.push(lat[:, a:b])
        assert len(fs._inflight) <= 2
        if len(views) >= 1:
            assert torch.equal(views[-1], seen[len(views) - 1])    # the latest delivered view has not been overwritten by this push
    fs.flush()
    assert len(seen) == 5 and not fs._inflight
    assert [f.shape[0] for f in seen] == [1, 4, 4, 4, 4 * (T - 4)]
    assert torch.equal(torch.cat(seen), want[0])
    assert fs.video() is None                                      # keep=False keeps nothing on the host


def test_reset_restarts_the_streams(tiny):
    from inferix_amd.streaming import FrameStream
    vae, lat, want, _, _ = tiny
    fs = FrameStream(vae, keep=True)
    for rnd in range(2):
        for a, b in cuts(lat.shape[1], (3,)):
            fs.push(lat[:, a:b])
        assert torch.equal(fs.video(), want), rnd
        assert fs.frames_pushed == want.shape[1]
        fs.reset()
        assert fs.video() is None and fs.frames_pushed == 0


def test_device_error_word_stops_delivery(tiny, monkeypatch):
    """The error word is read after a block's copy has completed and before it is delivered: with it raised, `flush()` raises, that
    block and the ones behind it are never delivered.  The word is raised by patching `hip_ops.check_device` (no fault is provoked)."""
    from inferix_amd import _hip, hip_ops
    from inferix_amd.streaming import FrameStream
    vae, lat, _, _, _ = tiny
    got = []
    fs = FrameStream(vae, slots=3, callback=got.append)
    fs.push(lat[:, :1])
    fs.flush()
    assert len(got) == 1
    calls = []

    def raised(what="", sync=False):
        calls.append(what)
        raise _hip.HipKernelError(f"{what}: a device-side wait gave up")
    monkeypatch.setattr(hip_ops, "check_device", raised)
    with pytest.raises(_hip.HipKernelError):
        fs.push(lat[:, 1:2])                                       # a push polls: whichever call sees the first finished copy raises
        fs.push(lat[:, 2:3])
        fs.flush()
    assert len(got) == 1 and calls and not fs._inflight
    fs.flush()                                                     # nothing left to deliver
    assert len(got) == 1


def test_needs_the_hip_decoder():
    from inferix_amd.streaming import FrameStream

    class Other:
        model = object()

        def decode_to_pixel(self, *a, **k):
            raise AssertionError("not reached")
    with pytest.raises(TypeError, match="continuous streaming needs the HIP decoder"):
        FrameStream(Other())
    with pytest.raises(TypeError, match="continuous streaming needs the HIP decoder"):
        FrameStream(object())

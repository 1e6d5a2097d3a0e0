"""GPU: `ifx_frames_yuv420` / `ifx_rgb8_yuv420` (`hip_ops.frames_yuv420`, `hip_ops.rgb8_to_yuv420`), bit for bit against the integer
restatement of tests/yuv_util.py: every bf16 value, every preset and layout, the vector and the general path at the same shapes with
guard bytes round the output, and more units than one pass of the capped grid covers."""
import pytest
import torch

import yuv_util as Y
from test_hip_frames import all_patterns

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LAYOUTS = ["i420", "nv12"]


def _entry(name):
    from inferix_amd import hip_ops
    return {"bf16": hip_ops.frames_yuv420, "rgb8": hip_ops.rgb8_to_yuv420}[name]


def test_every_bf16_value():
    """The 65 282 non-NaN patterns, padded to 65 536 with the first 254 again, as three differently permuted channel planes of one
    `[1, 128, 512, 3]` frame: Y sees every value in every channel, the chroma planes every value in some quad."""
    from inferix_amd import hip_ops
    from inferix_amd.streaming import yuv420_planes
    pats = all_patterns()
    pats = torch.cat([pats, pats[:65536 - pats.numel()]])
    g = torch.Generator().manual_seed(0)
    x = torch.stack([pats, pats[torch.randperm(65536, generator=g)], pats[torch.randperm(65536, generator=g)]], dim=-1)
    x = x.view(1, 128, 512, 3).contiguous()
    rgb = Y.bf16_to_u8(x)
    assert all(len(torch.unique(rgb[..., c])) == 256 for c in range(3))
    for layout in LAYOUTS:
        got = hip_ops.frames_yuv420(x.cuda(), layout=layout)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 192, 512)
        for name, a, b in zip("YUV", yuv420_planes(got.cpu(), layout), Y.planes(rgb)):
            assert torch.equal(a, b), (layout, name)


@pytest.fixture(scope="module")
def big_rgb():
    """`[1, 1024, 1024, 3]` random bytes with the eight cube corners and the 256 greys in constant 2 x 2 quads of the first quad row;
    computed once, shared, never written."""
    rgb = torch.randint(0, 256, (1, 1024, 1024, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    special = torch.cat([torch.tensor(Y.CORNERS, dtype=torch.uint8), torch.arange(256, dtype=torch.uint8).view(256, 1).expand(256, 3)])
    rgb[0, 0:2, :2 * len(special)] = special.repeat_interleave(2, dim=0)
    return rgb, rgb.cuda(), len(special)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix,full_range", Y.ALL_PRESETS)
def test_rgb8_every_preset_and_layout(big_rgb, matrix, full_range, layout):
    from inferix_amd import hip_ops
    from inferix_amd.streaming import yuv420_planes
    rgb, dev, n = big_rgb
    got = hip_ops.rgb8_to_yuv420(dev, layout=layout, matrix=matrix, full_range=full_range).cpu()
    assert torch.equal(got, Y.rgb_to_yuv420(rgb, layout, matrix, full_range))
    y, u, v = yuv420_planes(got, layout)
    assert bool((u[0, 0, 8:n] == 128).all()) and bool((v[0, 0, 8:n] == 128).all()), "the greys carry no chroma"
    hi = 255 if full_range else 240
    assert int(u[0, 0, 1]) == hi and int(v[0, 0, 4]) == hi, "blue and red reach the top (256 before the clamp in full range)"
    assert (int(y[0, 0, 0]), int(y[0, 0, 14])) == ((0, 255) if full_range else (16, 235))


def test_the_two_entry_points_agree_on_random_pixels():
    from inferix_amd import hip_ops
    x = (torch.randn(2, 64, 136, 3, generator=torch.Generator().manual_seed(2)) * 1.5).to(BF).cuda()
    assert float(x.max()) > 2 and float(x.min()) < -2
    u8 = hip_ops.frames_u8(x)
    for layout in LAYOUTS:
        for matrix, full_range in Y.ALL_PRESETS:
            a = hip_ops.frames_yuv420(x, layout=layout, matrix=matrix, full_range=full_range)
            b = hip_ops.rgb8_to_yuv420(u8, layout=layout, matrix=matrix, full_range=full_range)
            assert torch.equal(a, b), (layout, matrix, full_range)
    assert torch.equal(a.cpu(), Y.rgb_to_yuv420(u8.cpu(), "nv12", *Y.ALL_PRESETS[-1]))


@pytest.mark.parametrize("entry", ["bf16", "rgb8"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,H,W", [(1, 2, 2), (1, 2, 8), (2, 4, 10), (1, 2, 18), (3, 6, 24), (2, 4, 40)])
def test_geometry_alignment_and_guard_bytes(T, H, W, layout, entry):
    """Output views at byte offsets 0 .. 7 inside a buffer of 0xA5; input views at a 16-byte boundary and one pixel past it.  With
    w % 8 == 0 the aligned pair takes the vector path and every other pair the general one, at the same shape; the bytes are right
    and the guard bytes either side stay untouched."""
    fn = _entry(entry)
    matrix, full_range = Y.ALL_PRESETS[(T + H + W) % 4]         # the shapes go round the presets: each is met on both paths
    n_in, n_out, GUARD = T * H * W * 3, T * H * W * 3 // 2, 16
    g = torch.Generator().manual_seed(H * W)
    if entry == "bf16":
        pats = all_patterns()
        src = pats[torch.randint(0, pats.numel(), (n_in + 3,), generator=g)]
        rgb = Y.bf16_to_u8(src)
    else:
        src = rgb = torch.randint(0, 256, (n_in + 3,), generator=g, dtype=torch.uint8)
    dev = src.cuda()
    assert dev.data_ptr() % 16 == 0
    for xo in (0, 3):
        want = Y.rgb_to_yuv420(rgb[xo:xo + n_in].view(T, H, W, 3), layout, matrix, full_range).flatten()
        x = dev[xo:xo + n_in].view(T, H, W, 3)
        for yo in range(8):
            out = torch.full((GUARD + yo + n_out + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            assert out.data_ptr() % 8 == 0
            fn(x, out=out[GUARD + yo:GUARD + yo + n_out], layout=layout, matrix=matrix, full_range=full_range)
            got = out.cpu()
            assert torch.equal(got[GUARD + yo:GUARD + yo + n_out], want), (xo, yo)
            assert bool((got[:GUARD + yo] == 0xA5).all()) and bool((got[GUARD + yo + n_out:] == 0xA5).all()), (xo, yo)


def test_more_than_one_pass_of_the_grid():
    """Twelve 480 x 832 frames: 299 520 units of 2 x 8 pixels on the vector path and 1 198 080 quads on the general one, on a grid capped
    at 1024 x 256 lanes, so both grid-stride loops go round.  The restatement runs on the device here (integer torch, exact on either)."""
    from inferix_amd import hip_ops
    T, H, W = 12, 480, 832
    assert T * (H // 2) * (W // 8) > 1024 * 256
    x = torch.randn(T * H * W * 3 + 3, generator=torch.Generator().manual_seed(3)).to(BF).cuda()
    a, b = x[:-3].view(T, H, W, 3), x[3:].view(T, H, W, 3)
    for layout in LAYOUTS:
        assert torch.equal(hip_ops.frames_yuv420(a, layout=layout), Y.rgb_to_yuv420(Y.bf16_to_u8(a), layout)), layout
    assert torch.equal(hip_ops.frames_yuv420(b), Y.rgb_to_yuv420(Y.bf16_to_u8(b), "i420"))                 # one pixel past: general path
    u8 = torch.cat([hip_ops.frames_u8(a).flatten(), torch.zeros(3, dtype=torch.uint8, device="cuda")])
    a8, b8 = u8[:-3].view(T, H, W, 3), u8[3:].view(T, H, W, 3)
    assert torch.equal(hip_ops.rgb8_to_yuv420(a8, layout="nv12"), Y.rgb_to_yuv420(a8, "nv12"))
    want = Y.rgb_to_yuv420(b8, "nv12", "bt709", True)                                                      # uint8 general path
    assert torch.equal(hip_ops.rgb8_to_yuv420(b8, layout="nv12", matrix="bt709", full_range=True), want)


def test_nan_input_does_not_fault():
    """NaN is outside the contract: any byte may come out, the launch completes."""
    from inferix_amd import hip_ops
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = torch.stack([bits, bits.flip(0), bits.roll(77)], dim=-1).view(1, 128, 512, 3).contiguous().cuda()
    nan = torch.full((1, 4, 10, 3), float("nan"), dtype=BF, device="cuda")
    got = [hip_ops.frames_yuv420(x), hip_ops.frames_yuv420(x, layout="nv12"), hip_ops.frames_yuv420(nan)]
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (1, 192, 512) and tuple(got[2].shape) == (1, 6, 10)
    hip_ops.check_device("frames_yuv420 on NaNs")


def test_empty_block_and_wrapper_refusals_on_the_device():
    from inferix_amd import _hip, hip_ops
    e = hip_ops.frames_yuv420(torch.empty(0, 4, 6, 3, dtype=BF, device="cuda"))
    assert tuple(e.shape) == (0, 6, 6) and e.dtype == torch.uint8
    x = torch.zeros(1, 4, 6, 3, dtype=BF, device="cuda")
    with pytest.raises(TypeError):
        hip_ops.frames_yuv420(x.float())
    with pytest.raises(TypeError):
        hip_ops.rgb8_to_yuv420(x)
    with pytest.raises(TypeError):
        hip_ops.frames_yuv420(x, out=torch.empty(1, 6, 6, dtype=torch.int8, device="cuda"))
    with pytest.raises(_hip.HipKernelError):
        hip_ops.frames_yuv420(x.cpu())
    with pytest.raises(ValueError, match="even frame size, got 3 x 6"):
        hip_ops.rgb8_to_yuv420(torch.zeros(1, 3, 6, 3, dtype=torch.uint8, device="cuda"))

"""GPU: `ifx_vit_tile_blend_hwc`, the channel-last uint8 output of the MAGI tile blend, against the planar uint8 output of
`ifx_vit_tile_blend` (itself bit-exact against the reference-generated fixtures, tests/test_hip_magi_tiles.py): the two must hold the same
bytes, `hwc == planar.view(N, T, 3, H, W).permute(0, 1, 3, 4, 2)`, on every fixture geometry and on made-up ones, on both lane layouts;
nothing outside the output is written; the argument checks answer before any launch; and `tiled_decode_3d(uint8_output="hwc")`."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import pytest
import torch

import magi_tiles_util as TU
from test_hip_magi_tiles import NAMES, _cpu, _fill, _plan, _vae

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 0xA5


def _both(desc, arena):
    """(planar uint8 permuted to channel-last, channel-last uint8) of one arena, on the CPU."""
    from inferix_amd import hip_ops as ops
    table = desc.tensor(arena.device)
    _, planar = ops.vit_tile_blend(arena, desc, table, out=False, out_u8=True)
    none, none_u8, hwc = ops.vit_tile_blend(arena, desc, table, out=False, out_hwc=True)
    torch.cuda.synchronize()
    T, H, W = desc.out_shape
    assert none is None and none_u8 is None and hwc.dtype == torch.uint8 and tuple(hwc.shape) == (desc.batch, T, H, W, 3)
    return planar.view(desc.batch, T, 3, H, W).permute(0, 1, 3, 4, 2).cpu(), hwc.cpu()


def _made_up(batch, extents, blends, limits, seed, frame_pitch=None, align=8):
    """A descriptor that no decoder need produce, random tiles, the restated blends in torch: (desc, arena, expected planar frames)."""
    from inferix_amd.magi.tiles import blend_table
    starts = tuple(tuple(sum(min(x, lim) for x in ext[:k]) for k in range(len(ext))) for ext, lim in zip(extents, limits))
    out_shape = tuple(s[-1] + min(e[-1], lim) for s, e, lim in zip(starts, extents, limits))
    g = torch.Generator().manual_seed(seed)
    raw = {(a, b, c): torch.randn(batch, 3, extents[0][a], extents[1][b], extents[2][c], generator=g).to(BF)
           for a in range(len(extents[0])) for b in range(len(extents[1])) for c in range(len(extents[2]))}
    axes = [SimpleNamespace(count=len(e), extent=b, limit=lim) for e, b, lim in zip(extents, blends, limits)]
    want = TU.uint8_frames(TU.blend_tiles(raw, axes))
    desc = blend_table(batch, extents, starts, blends, limits, out_shape, frame_pitch=frame_pitch, align=align)
    return desc, _fill(desc, raw), want


def _hwc_of(frames, batch):
    NT, _, H, W = frames.shape
    return frames.view(batch, NT // batch, 3, H, W).permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize("name", NAMES)
def test_hwc_equals_the_planar_frames_on_every_fixture_geometry_on_both_paths(name):
    from inferix_amd.magi.tiles import plan_blend_table
    want, raw, _ = _cpu(name)
    batch = TU.CASES[name][0]
    desc = plan_blend_table(_plan(name), batch)
    assert desc.vec_x
    arena = _fill(desc, raw)
    planar, hwc = _both(desc, arena)
    assert torch.equal(hwc, planar), f"{name}: {int((hwc != planar).sum())} bytes differ on the 8-pixel path"
    assert torch.equal(hwc, _hwc_of(TU.uint8_frames(want), batch)), f"{name}: differs from the reference's frames"
    planar1, hwc1 = _both(dataclasses.replace(desc, vec_x=False), arena)            # the same geometry a second time, one pixel per lane
    assert torch.equal(hwc1, planar1) and torch.equal(hwc1, hwc), f"{name}: scalar path"


def test_hwc_on_a_geometry_with_odd_widths():
    """The geometry of test_blend_kernel_scalar_path_on_a_geometry_with_odd_widths: x extents that are no multiples of 8, batch 2."""
    desc, arena, want = _made_up(2, ((3, 2), (10, 10, 5), (13, 13, 6)), (1, 3, 5), (2, 7, 8), seed=31, align=1)
    assert desc.out_shape == (4, 19, 22) and not desc.vec_x and any(o % 8 for o in desc.offsets)
    planar, hwc = _both(desc, arena)
    assert torch.equal(hwc, planar) and torch.equal(hwc, _hwc_of(want, 2))


@pytest.mark.parametrize("vec_x", [True, False])
def test_hwc_of_a_chunk_of_one_latent_frame_keeps_one_frame_of_the_pitch(vec_x):
    """One temporal tile of extent 1 whose storage holds patch_t = 4 frames (what the decoder writes for a single latent frame), 2 x 2
    spatial tiles; the three frames behind the tile are NaN in the arena."""
    desc, arena, want = _made_up(1, ((1,), (24, 16), (32, 16)), (0, 8, 8), (4, 16, 24), seed=32, frame_pitch=(4,))
    assert desc.out_shape == (1, 32, 40) and desc.vec_x and desc.frame_pitch == (4,)
    planar, hwc = _both(dataclasses.replace(desc, vec_x=vec_x), arena)
    assert torch.equal(hwc, planar) and torch.equal(hwc, _hwc_of(want, 1))


@pytest.mark.parametrize("vec_x", [True, False])
def test_hwc_of_a_chunk_smaller_than_a_tile_has_no_blend(vec_x):
    """One tile on every axis: no neighbour, the frames are the tile's own values; more than one block per frame (48 x 56 pixels)."""
    desc, arena, want = _made_up(2, ((3,), (48,), (56,)), (2, 8, 8), (8, 64, 64), seed=33)
    assert desc.grid == (1, 1, 1) and desc.out_shape == (3, 48, 56) and desc.vec_x
    planar, hwc = _both(dataclasses.replace(desc, vec_x=vec_x), arena)
    assert torch.equal(hwc, planar) and torch.equal(hwc, _hwc_of(want, 2))


@pytest.mark.parametrize("vec_x", [True, False])
def test_hwc_writes_nothing_outside_its_output(vec_x):
    """The output in the middle of a larger byte buffer of sentinels (at an 8-byte aligned offset; one byte further on the scalar path):
    every byte outside `batch t_out h_out w_out 3` is unchanged."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.tiles import plan_blend_table
    name = "magi_tiles_b"
    want, raw, _ = _cpu(name)
    batch = TU.CASES[name][0]
    desc = dataclasses.replace(plan_blend_table(_plan(name), batch), vec_x=vec_x)
    arena = _fill(desc, raw)
    T, H, W = desc.out_shape
    n = batch * T * H * W * 3
    lead = 4096 if vec_x else 4097
    buf = torch.full((lead + n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    out = buf[lead:lead + n].view(batch, T, H, W, 3)
    got = ops.vit_tile_blend(arena, desc, desc.tensor(arena.device), out=False, out_hwc=out)[2]
    torch.cuda.synchronize()
    assert got is out
    host = buf.cpu()
    assert bool((host[:lead] == SENTINEL).all()) and bool((host[lead + n:] == SENTINEL).all()), "bytes outside the output were written"
    assert torch.equal(host[lead:lead + n].view(batch, T, H, W, 3), _hwc_of(TU.uint8_frames(want), batch))


def test_hwc_argument_errors_answer_before_any_launch():
    """Null `out_hwc`, a misaligned `out_hwc` on the vec_x path and `t_out` / `batch` > 65535 return IFX_EINVAL through the C-ABI (dummy
    pointers: a launch would fault, a refusal touches nothing); the sibling's checks are there too."""
    from inferix_amd import _hip
    lib = _hip.load()
    P, P4, P1 = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4097)
    EINVAL = -1

    def refused(rc, *parts):
        msg = lib.ifx_last_error()
        assert rc == EINVAL and all(p in msg for p in parts), (rc, msg)

    # (arena, table, out_hwc, batch, T, H, W, nt, nh, nw, et, eh, ew, lt, lh, lw, vec_x, stream): fixture a's geometry
    blend = lambda arena=P, table=P, out=P, batch=1, T=9, H=56, W=40, nt=2, nh=3, nw=2, et=0, eh=8, ew=8, lt=8, lh=24, lw=24, vec=1: \
        lib.ifx_vit_tile_blend_hwc(arena, table, out, batch, T, H, W, nt, nh, nw, et, eh, ew, lt, lh, lw, vec, None)
    refused(blend(out=None), b"ifx_vit_tile_blend_hwc", b"null out_hwc")
    refused(blend(out=P4), b"ifx_vit_tile_blend_hwc", b"out_hwc 8-byte aligned")
    refused(blend(out=P1), b"ifx_vit_tile_blend_hwc", b"out_hwc 8-byte aligned")
    refused(blend(T=70000, nt=10000), b"ifx_vit_tile_blend_hwc", b"launch too large", b"70000 frames")
    refused(blend(batch=65536), b"ifx_vit_tile_blend_hwc", b"launch too large", b"65536 samples")
    refused(blend(arena=None), b"ifx_vit_tile_blend_hwc", b"null arena")
    refused(blend(table=None), b"ifx_vit_tile_blend_hwc", b"null arena / table")
    refused(blend(batch=0), b"ifx_vit_tile_blend_hwc", b"empty output (0 x 9 x 56 x 40)")
    refused(blend(W=0), b"ifx_vit_tile_blend_hwc", b"empty output")
    refused(blend(nh=0), b"ifx_vit_tile_blend_hwc", b"empty tile grid (2 x 0 x 2)")
    refused(blend(ew=32), b"ifx_vit_tile_blend_hwc", b"larger than its limit (8, 24, 24)")
    refused(blend(H=80), b"ifx_vit_tile_blend_hwc", b"h_out (80)", b"3 tiles of limit 24")
    refused(blend(table=P4), b"ifx_vit_tile_blend_hwc", b"table", b"8-byte")
    refused(blend(W=36), b"ifx_vit_tile_blend_hwc", b"vec_x", b"w_out (36)")
    refused(blend(arena=C.c_void_p(4104)), b"ifx_vit_tile_blend_hwc", b"arena 16-byte")
    refused(blend(arena=P1, vec=0), b"ifx_vit_tile_blend_hwc", b"2-byte")


def test_hwc_wrapper_refuses_a_wrong_shape():
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.tiles import plan_blend_table
    desc = plan_blend_table(_plan("magi_tiles_a"), 1)
    arena = torch.zeros(desc.arena_elements, dtype=BF, device="cuda")
    T, H, W = desc.out_shape
    with pytest.raises(AssertionError):
        ops.vit_tile_blend(arena, desc, desc.tensor("cuda"), out=False, out_hwc=torch.empty(T, 3, H, W, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("name", ["magi_tiles_b", "magi_tiles_d"])
def test_decoder_hwc_output_equals_the_planar_frames_permuted(name):
    from inferix_amd.magi.vae import VaeHelper
    vae = _vae()
    z = TU.case_input(name).cuda()
    kw = TU.case_kwargs(name)
    u8 = vae.tiled_decode_3d(z, **kw, uint8_output=True)
    hwc = vae.tiled_decode_3d(z, **kw, uint8_output="hwc")
    N = z.shape[0]
    want = _hwc_of(u8, N)
    assert hwc.dtype == torch.uint8 and hwc.shape == want.shape and hwc.is_contiguous() and torch.equal(hwc, want)
    out = torch.full_like(hwc, SENTINEL)
    assert vae.tiled_decode_3d(z, **kw, uint8_output=out) is out and torch.equal(out, want)              # a tensor to fill
    out.fill_(SENTINEL)
    assert VaeHelper.decode(z, vae, **kw, uint8_output=out) is out and torch.equal(out, want)
    assert torch.equal(VaeHelper.decode(z, vae, **kw, uint8_output="hwc"), want)
    assert torch.equal(vae.tiled_decode_3d(z, **kw, uint8_output=True), u8), "the planar form is as it was"
    with pytest.raises(ValueError, match="uint8_output"):
        vae.tiled_decode_3d(z, **kw, uint8_output="chw")
    with pytest.raises(AssertionError):
        vae.tiled_decode_3d(z, **kw, uint8_output=out[:, :-1])

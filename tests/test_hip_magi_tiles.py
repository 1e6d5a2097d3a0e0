"""GPU: the tiled chunk decode of MAGI's ViT-VAE — `ifx_vit_tile_blend` teacher-forced and bit-exact against the reference-generated
fixtures tests/golden/magi_tiles_*.npz, then `HipMagiVAEDecoder.tiled_decode_3d` end to end under the measured-noise rule (the float32
evaluation of the restatement is the exact answer, the fixture sits `floor` (rel-L2) from it, HIP must be within 1.25 x floor of the
exact answer and 2 x floor of the fixture), and bit for bit against a tile-by-tile loop of `decode` with the restated blends on the device.
Fixtures and seeds only."""
import dataclasses
import functools
from types import SimpleNamespace

import pytest
import torch

import magi_tiles_util as TU
import magi_vit_util as U
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAMES = sorted(TU.CASES)
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _weights(dtype=BF):
    return U.make_weights(U.TINY, TU.WEIGHT_SEED, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _vae():
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    vae = HipMagiVAEDecoder(U.TINY.ctor_kwargs(), device="cuda:0")
    vae.load_state_dict({"decoder." + k: v for k, v in _weights().items()})
    return vae


@functools.lru_cache(maxsize=None)
def _cpu(name):
    """(fixture output, the raw tiles the reference's `decode` returned on the CPU, the axes): loaded once, shared, never written to.  The
    tiles come from the fixture, not from `decoder_forward` here: torch's bf16 products on a CPU depend on its instruction set."""
    axes = TU.case_axes(name)
    return U.load_fixture(name)["out"], TU.load_raw_tiles(name, axes), axes


@functools.lru_cache(maxsize=None)
def _plan(name):
    from inferix_amd.magi.tiles import plan_tiles
    _, latent, (tl, th, tw), fs, ft, _, _ = TU.CASES[name]
    return plan_tiles(latent, tl, th, tw, fs, ft, 8, 4)


def _fill(desc, raw, spoil=None):
    """An arena of NaN with the raw tiles at the descriptor's offsets (a tile's storage holds `frame_pitch` frames, the tile in the first
    ones); `spoil(tile)` may overwrite parts of a copy of each tile."""
    arena = torch.full((desc.arena_elements,), NAN, dtype=BF)
    nt, nh, nw = desc.grid
    for (it, ih, iw), tile in raw.items():
        tile = tile.clone()
        if spoil is not None:
            spoil(tile)
        N, C, T, H, W = tile.shape
        off = desc.offsets[(it * nh + ih) * nw + iw]
        slot = arena[off:off + N * C * desc.frame_pitch[it] * H * W].view(N, C, desc.frame_pitch[it], H, W)
        slot[:, :, :T] = tile
    return arena.cuda()


def _launch(desc, arena, **kw):
    from inferix_amd import hip_ops as ops
    out, u8 = ops.vit_tile_blend(arena, desc, desc.tensor(arena.device), **kw)
    torch.cuda.synchronize()
    return (None if out is None else out.cpu()), (None if u8 is None else u8.cpu())


@pytest.mark.parametrize("name", NAMES)
def test_blend_kernel_teacher_forced_bit_exact(name):
    from inferix_amd.magi.tiles import plan_blend_table
    want, raw, _ = _cpu(name)
    want_u8 = TU.uint8_frames(want)
    batch = TU.CASES[name][0]
    desc = plan_blend_table(_plan(name), batch)
    assert desc.vec_x
    arena = _fill(desc, raw)
    out, none = _launch(desc, arena, out=True, out_u8=False)
    assert none is None and out.dtype == BF and torch.equal(out, want), f"{name}: bf16 output differs from the reference's"
    none, u8 = _launch(desc, arena, out=False, out_u8=True)
    assert none is None and u8.dtype == torch.uint8 and u8.shape == want_u8.shape and torch.equal(u8, want_u8), f"{name}: uint8 frames"
    both, both_u8 = _launch(desc, arena, out=True, out_u8=True)
    assert torch.equal(both, out) and torch.equal(both_u8, u8), f"{name}: both outputs in one launch"
    # the one-pixel-per-lane path on the same geometry
    out1, u81 = _launch(dataclasses.replace(desc, vec_x=False), arena, out=True, out_u8=True)
    assert torch.equal(out1, want) and torch.equal(u81, want_u8), f"{name}: scalar path"


@pytest.mark.parametrize("name", NAMES)
def test_blend_kernel_reads_nothing_beyond_the_limit_on_two_axes(name):
    """NaN wherever no formula reads: past the limit on two axes at once, in the frames a single-frame tile's storage holds behind the
    tile, and between the tiles."""
    from inferix_amd.magi.tiles import plan_blend_table
    want, raw, axes = _cpu(name)
    lt, lh, lw = (a.limit for a in axes)
    plan = _plan(name)
    pitch = tuple(4 * (e - b) for b, e in plan.axes[0].spans)          # what the decoder writes: 4 frames for one latent frame

    def spoil(tile):
        tile[:, :, lt:, lh:, :] = NAN
        tile[:, :, lt:, :, lw:] = NAN
        tile[:, :, :, lh:, lw:] = NAN

    desc = plan_blend_table(plan, TU.CASES[name][0], frame_pitch=pitch)
    out, u8 = _launch(desc, _fill(desc, raw, spoil), out=True, out_u8=True)
    assert torch.equal(out, want) and torch.equal(u8, TU.uint8_frames(want)), name


def test_blend_kernel_scalar_path_on_a_geometry_with_odd_widths():
    """x extents that are no multiples of 8 (no decoder produces them: the descriptor is made up), random tiles, batch 2; against the
    restated blends in torch."""
    from inferix_amd.magi.tiles import blend_table
    extents = ((3, 2), (10, 10, 5), (13, 13, 6))
    blends, limits = (1, 3, 5), (2, 7, 8)
    starts = tuple(tuple(sum(min(x, lim) for x in ext[:k]) for k in range(len(ext))) for ext, lim in zip(extents, limits))
    out_shape = tuple(s[-1] + min(e[-1], lim) for s, e, lim in zip(starts, extents, limits))
    assert out_shape == (4, 19, 22)
    g = torch.Generator().manual_seed(31)
    raw = {(a, b, c): torch.randn(2, 3, extents[0][a], extents[1][b], extents[2][c], generator=g).to(BF)
           for a in range(2) for b in range(3) for c in range(3)}
    axes = [SimpleNamespace(count=len(e), extent=b, limit=lim) for e, b, lim in zip(extents, blends, limits)]
    want = TU.blend_tiles(raw, axes)
    assert tuple(want.shape) == (2, 3) + out_shape
    desc = blend_table(2, extents, starts, blends, limits, out_shape, align=1)
    assert not desc.vec_x and any(o % 8 for o in desc.offsets)
    out, u8 = _launch(desc, _fill(desc, raw), out=True, out_u8=True)
    assert torch.equal(out, want) and torch.equal(u8, TU.uint8_frames(want))


@pytest.mark.parametrize("name", NAMES)
def test_tiled_decode_end_to_end_measured_noise(name):
    want, _, _ = _cpu(name)
    exact = TU.tiled_decode_restated(TU.tiny_decode(_weights(torch.float32)), TU.case_input(name, torch.float32), **TU.case_kwargs(name))
    floor = rel_l2(want, exact)
    out = _vae().tiled_decode_3d(TU.case_input(name).cuda(), **TU.case_kwargs(name)).cpu()
    assert out.shape == want.shape and out.dtype == BF and torch.isfinite(out.float()).all()
    err_exact, err_ref = rel_l2(out, exact), rel_l2(out, want)
    line = f"{name}: bf16 floor {floor:.3e}, HIP vs float32 {err_exact:.3e} (bound {1.25 * floor:.3e}), HIP vs reference {err_ref:.3e} (bound {2 * floor:.3e})"
    print(line)
    assert err_exact <= 1.25 * floor and err_ref <= 2.0 * floor, line


@pytest.mark.parametrize("max_rows", [1, None])
@pytest.mark.parametrize("name", NAMES)
def test_batched_groups_equal_tile_by_tile_bit_for_bit(name, max_rows):
    """`tiled_decode_3d` against a loop of `vae.decode(tile)` and the restated blends in torch on the device; max_rows 1 forces one tile
    per forward, the default batches every group."""
    vae = _vae()
    z = TU.case_input(name).cuda()
    want = TU.tiled_decode_restated(vae.decode, z, **TU.case_kwargs(name))
    got = vae.tiled_decode_3d(z, **TU.case_kwargs(name), max_rows_per_forward=max_rows)
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} values differ"


def test_batched_groups_equal_tile_by_tile_at_the_published_width():
    """Two blocks of width 1024 x 16 heads, ln_in_attn, final projection, synthetic weights: four-tile groups of 4097 tokens, edge tiles
    of 8 latents, the T == 1 rule (1025-token tiles) at real width."""
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    cfg = U.VitConfig(video_size=256, video_length=16, z_chans=16, embed_dim=1024, depth=2, num_heads=16, qkv_bias=True, ln_in_attn=True,
                      use_final_proj=True)
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda:0")
    vae.decoder.load_synthetic(seed=5)
    z = torch.randn(1, 16, 5, 56, 56, generator=torch.Generator().manual_seed(6)).to(BF).cuda()
    kw = dict(tile_sample_min_length=16, tile_sample_min_height=256, tile_sample_min_width=256, allow_spatial_tiling=True)
    plan = vae.tile_plan(z.shape, **kw)
    groups = {k: len(v) for k, v in plan.groups().items()}
    assert groups[(4, 32, 32)] == 4 and groups[(1, 32, 32)] == 4 and groups[(4, 8, 8)] == 1 and len(plan.tiles) == 18
    want = TU.tiled_decode_restated(vae.decode, z, **kw)
    got = vae.tiled_decode_3d(z, **kw)
    assert tuple(got.shape) == (1, 3, 17, 448, 448) and torch.isfinite(got.float()).all()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} values differ"


def test_batch_two_equals_two_single_calls_and_calls_are_deterministic():
    vae = _vae()
    kb, ka, kc = (TU.case_kwargs(n) for n in ("magi_tiles_b", "magi_tiles_a", "magi_tiles_c"))
    zb = TU.case_input("magi_tiles_b").cuda()
    both = vae.tiled_decode_3d(zb, **kb)
    for i in range(2):
        assert torch.equal(both[i:i + 1], vae.tiled_decode_3d(zb[i:i + 1], **kb)), f"sample {i} of a batch of 2"
    za, zc = TU.case_input("magi_tiles_a").cuda(), TU.case_input("magi_tiles_c").cuda()
    first = vae.tiled_decode_3d(za, **ka)
    cached = len(vae._tile_cache)
    other = vae.tiled_decode_3d(zc, **kc)                    # another geometry in between: its own plan and arena
    again = vae.tiled_decode_3d(za, **ka)
    assert torch.equal(first, again) and torch.equal(other, vae.tiled_decode_3d(zc, **kc))
    assert len(vae._tile_cache) >= 2 and len(vae._tile_cache) >= cached and first.data_ptr() != again.data_ptr()
    n = len(vae._tile_cache)
    vae.tiled_decode_3d(za, **ka)
    assert len(vae._tile_cache) == n, "a repeated call builds no new plan"


def test_a_chunk_smaller_than_a_tile_equals_decode():
    vae = _vae()
    z = TU.case_input("magi_tiles_a").cuda()                 # 3 x 7 x 5 latents, tiles of 4 x 32 x 32
    assert torch.equal(vae.tiled_decode_3d(z, allow_spatial_tiling=True), vae.decode(z))
    assert torch.equal(vae.tiled_decode_3d(z), vae.decode(z))                         # no spatial tiling: one tile of any frame size
    one = vae.tiled_decode_3d(z[:, :, :1])
    assert one.shape[2] == 1 and torch.equal(one, vae.decode(z[:, :, :1]))            # the T == 1 rule through the frame pitch


@pytest.mark.parametrize("name", ["magi_tiles_b", "magi_tiles_d"])
def test_uint8_output_equals_the_chain_on_the_bf16_result(name):
    from inferix.pipeline.magi.video_process import VaeHelper
    vae = _vae()
    z = TU.case_input(name).cuda()
    bf = vae.tiled_decode_3d(z, **TU.case_kwargs(name))
    u8 = vae.tiled_decode_3d(z, **TU.case_kwargs(name), uint8_output=True)
    want = TU.uint8_frames(bf.cpu())
    assert u8.dtype == torch.uint8 and u8.shape == want.shape and torch.equal(u8.cpu(), want)
    kw = {k: v for k, v in TU.case_kwargs(name).items()}
    assert torch.equal(VaeHelper.decode(z, vae, **kw).cpu(), want)
    frames = VaeHelper.decode(z, vae, uint8_output=False, **kw)
    assert frames.dtype == BF and torch.equal(frames, bf.permute(0, 2, 1, 3, 4).reshape(frames.shape))

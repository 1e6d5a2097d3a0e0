"""CPU: the MAGI tiled chunk decode fixtures, the tile plan and the host side of `ifx_vit_tile_blend`.  tests/golden/magi_tiles_*.npz hold
what the reference's own `ViTVAE.tiled_decode_3d` computed on the CPU in bf16 (tools/gen_golden_magi_tiles.py); the first test guards
them against the restatement tests/magi_tiles_util.py, the others fail without the plan, the kernel's entry point, the bindings and the
shims."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import magi_tiles_util as TU
import magi_vit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.fixture(scope="module")
def tiny_weights():
    return U.make_weights(U.TINY, TU.WEIGHT_SEED)


@pytest.mark.parametrize("name", sorted(TU.CASES))
def test_restatement_reproduces_the_reference_fixture_bit_for_bit(name, tiny_weights):
    batch, latent, tile_px, fs, ft, xseed, out_shape = TU.CASES[name]
    fx = U.load_fixture(name)
    assert int(fx["weight_seed"]) == TU.WEIGHT_SEED and int(fx["input_seed"]) == xseed and int(fx["batch"]) == batch
    assert tuple(fx["latent"].tolist()) == latent and tuple(fx["tile_sample_min"].tolist()) == tile_px
    assert fx["overlap_factors"].tolist() == [fs, ft]
    out = TU.tiled_decode_restated(TU.tiny_decode(tiny_weights), TU.case_input(name), **TU.case_kwargs(name))
    assert out.dtype == BF and tuple(out.shape) == (batch, 3) + out_shape and torch.equal(out, fx["out"]), name


@pytest.mark.parametrize("name", sorted(TU.CASES))
def test_restated_blends_of_the_recorded_raw_tiles_give_the_fixture(name):
    axes = TU.case_axes(name)
    raw = TU.load_raw_tiles(name, axes)
    fx = U.load_fixture(name)
    assert [tuple(t.shape[2:]) for t in raw.values()] == [(1 if s[2] == 1 else 4 * s[2], 8 * s[3], 8 * s[4]) for s in fx["decode_shapes"].tolist()]
    assert torch.equal(TU.blend_tiles(raw, axes), fx["out"]), name


@pytest.mark.parametrize("name", sorted(TU.CASES))
def test_plan_reproduces_the_recorded_tiles_of_the_reference(name):
    from inferix_amd.magi.tiles import plan_tiles
    batch, latent, (tl, th, tw), fs, ft, _, out_shape = TU.CASES[name]
    fx = U.load_fixture(name)
    plan = plan_tiles(latent, tl, th, tw, fs, ft, 8, 4)
    recorded = [tuple(s) for s in fx["decode_shapes"].tolist()]
    assert [(batch, 4) + plan.latent_shape(idx) for idx in plan.tiles] == recorded          # shapes in the reference's call order
    assert plan.out_shape == out_shape == tuple(fx["out"].shape[2:])
    nt, nh, nw = plan.grid
    assert list(plan.tiles) == [(a, b, c) for a in range(nt) for b in range(nh) for c in range(nw)]
    for idx in plan.tiles:                    # the T == 1 rule: one latent frame decodes to one pixel frame
        lt, lh, lw = plan.latent_shape(idx)
        assert plan.decoded_shape(idx) == (1 if lt == 1 else 4 * lt, 8 * lh, 8 * lw)


def test_plan_details_of_the_fixture_geometries():
    from inferix_amd.magi.tiles import plan_tiles
    a = plan_tiles((3, 7, 5), 8, 32, 32, 0.25, 0.0, 8, 4)
    assert a.grid == (2, 3, 2) and a.axes[0].extents == (8, 1) and a.axes[1].extents == (32, 32, 8) and a.axes[2].extents == (32, 16)
    assert [x.blend for x in a.axes] == [0, 8, 8] and [x.limit for x in a.axes] == [8, 24, 24] and a.axes[1].starts == (0, 24, 48)
    b = plan_tiles((2, 4, 3, 7, 5), 8, 32, 32, 0.25, 0.5, 8, 4)
    assert b.grid == (3, 3, 2) and b.axes[0].extents == (8, 8, 1) and b.axes[0].blend == 4 and b.axes[0].limit == 4
    assert b.axes[0].blend_extent(2) == 1 and b.axes[0].blend_extent(1) == 4 and b.axes[0].blend_extent(0) == 0
    c = plan_tiles((3, 14, 11), 8, 96, 96, 0.25, 0.0, 8, 4)
    assert c.axes[2].blend == 24 and c.axes[2].extents == (88, 16) and c.axes[1].extents == (96, 40) and c.axes[2].blend_extent(1) == 16       # the `min` rule
    d = plan_tiles((5, 7, 11), 16, 32, 96, 0.25, 0.25, 8, 4)
    assert d.axes[0].blend == 4 and d.axes[0].limit == 12 and d.grid == (2, 3, 2)


def test_plan_at_the_config5_chunk_geometry():
    from inferix_amd.magi.tiles import plan_blend_table, plan_tiles
    plan = plan_tiles((1, 16, 6, 90, 90), 12, 256, 256, 0.25, 0, 8, 4)
    assert len(plan.tiles) == 32 and plan.grid == (2, 4, 4) and plan.out_shape == (24, 720, 720)
    groups = plan.groups()
    assert {k: len(v) for k, v in groups.items()} == {(3, 32, 32): 18, (3, 32, 18): 6, (3, 18, 32): 6, (3, 18, 18): 2}
    assert [x.blend for x in plan.axes] == [0, 64, 64] and [x.limit for x in plan.axes] == [12, 192, 192]
    desc = plan_blend_table(plan, 1)
    # offsets, extents + starts, frame pitches, then tiles x extent weight words per axis
    assert desc.vec_x and len(desc.words) == 32 + 2 * (2 + 4 + 4) + 2 + (2 * 0 + 4 * 64 + 4 * 64) and desc.out_shape == (24, 720, 720)
    pixels, reads = plan.traffic_elements(1)
    # own pixels + the 64-wide blend strips of the 3 inner seams per axis
    assert pixels == 3 * 24 * 720 * 720 and reads == pixels + 2 * 3 * 24 * 720 * 3 * 64
    from inferix_amd.magi.vae import MAX_ROWS_PER_FORWARD
    assert 18 * (3 * 32 * 32 + 1) <= MAX_ROWS_PER_FORWARD, "the largest config-5 group runs unsplit by default"


def test_a_chunk_smaller_than_one_tile_is_a_single_tile_with_no_blend():
    from inferix_amd.magi.tiles import plan_tiles
    plan = plan_tiles((2, 5, 7), 16, 256, 256, 0.25, 0, 8, 4)
    assert plan.tiles == ((0, 0, 0),) and plan.latent_shape((0, 0, 0)) == (2, 5, 7) and plan.out_shape == (8, 40, 56)
    assert all(x.blend_extent(0) == 0 for x in plan.axes)
    assert plan_tiles((1, 5, 7), 16, 100000, 100000, 0.25, 0, 8, 4).out_shape == (1, 40, 56)


def test_plan_refuses_a_geometry_whose_concatenation_does_not_line_up():
    from inferix_amd.magi.tiles import plan_tiles
    with pytest.raises(NotImplementedError, match=r"4 latents = 32 px.*keep 36 px"):
        plan_tiles((2, 12, 4), 8, 48, 32, 0.25, 0, 8, 4)
    assert plan_tiles((2, 4, 3), 8, 48, 32, 0.25, 0, 8, 4).grid == (1, 1, 1)         # a single tile on that axis: nothing to line up
    with pytest.raises(ValueError, match="stride"):
        plan_tiles((2, 4, 4), 8, 32, 32, 1.0, 0, 8, 4)


def test_decoder_refusals_and_the_spatial_tiling_rule():
    from inferix_amd import _hip
    from inferix_amd.magi.vae import HipMagiVAEDecoder, VaeHelper
    vae = HipMagiVAEDecoder(U.TINY.ctor_kwargs(), device="cpu")
    assert vae.allow_spatial_tiling is False
    z = torch.zeros(1, 4, 2, 8, 8, dtype=BF)
    with pytest.raises(NotImplementedError, match="parallel_group"):
        vae.tiled_decode_3d(z, parallel_group=object())
    with pytest.raises(NotImplementedError, match="encoder"):
        vae.tiled_encode_3d(z)
    with pytest.raises(_hip.HipKernelError):
        vae.tiled_decode_3d(z)
    with pytest.raises(NotImplementedError, match="parallel_group"):
        VaeHelper.decode(z, vae, parallel_group=object())
    with pytest.raises(TypeError):
        VaeHelper.decode(z, object())
    # allow_spatial_tiling=None falls back to the property (False): the spatial tile is 100000 px, one tile whatever the frame size
    kw = dict(tile_sample_min_height=32, tile_sample_min_width=32, tile_sample_min_length=8)
    assert vae.tile_plan(z.shape, **kw).grid == vae.tile_plan(z.shape, allow_spatial_tiling=False, **kw).grid == (1, 1, 1)
    assert vae.tile_plan(z.shape, **kw).axes[1].tile == 100000 // 8
    assert vae.tile_plan(z.shape, allow_spatial_tiling=True, **kw).grid == (1, 3, 3)
    sig = inspect.signature(HipMagiVAEDecoder.tiled_decode_3d).parameters
    assert [(k, p.default) for k, p in sig.items()][2:] == [
        ("tile_sample_min_height", 256), ("tile_sample_min_width", 256), ("tile_sample_min_length", 16), ("spatial_tile_overlap_factor", 0.25),
        ("temporal_tile_overlap_factor", 0), ("allow_spatial_tiling", None), ("verbose", False), ("parallel_group", None),
        ("uint8_output", False), ("max_rows_per_forward", None)]


def test_tile_blend_export_is_declared_bound_and_exported_without_an_abi_bump():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    lib = _hip.load()
    _vp, _i32 = C.c_void_p, C.c_int32
    args = [_vp, _vp, _vp, _vp] + [_i32] * 14 + [_vp]
    decl = re.search(r"\bint ifx_vit_tile_blend\(([^;]*)\);", hdr)
    assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == len(args)
    assert _hip.SIGNATURES["ifx_vit_tile_blend"] == (C.c_int, args) and lib.ifx_vit_tile_blend is not None
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)


def test_tile_blend_argument_validation_without_gpu():
    """Every argument check of ifx_vit_tile_blend answers before any launch (dummy aligned pointers, no GPU): code and message."""
    from inferix_amd import _hip
    lib = _hip.load()
    P, P8, P1 = C.c_void_p(4096), C.c_void_p(4104), C.c_void_p(4097)
    EINVAL = -1

    def refused(rc, *parts):
        msg = lib.ifx_last_error()
        assert rc == EINVAL and all(p in msg for p in parts), (rc, msg)

    # (arena, table, out, out_u8, batch, T, H, W, nt, nh, nw, et, eh, ew, lt, lh, lw, vec_x, stream): fixture a's geometry
    blend = lambda arena=P, table=P, out=P, u8=P, batch=1, T=9, H=56, W=40, nt=2, nh=3, nw=2, et=0, eh=8, ew=8, lt=8, lh=24, lw=24, vec=1: \
        lib.ifx_vit_tile_blend(arena, table, out, u8, batch, T, H, W, nt, nh, nw, et, eh, ew, lt, lh, lw, vec, None)
    refused(blend(arena=None), b"ifx_vit_tile_blend", b"null arena")
    refused(blend(table=None), b"ifx_vit_tile_blend", b"null arena / table")
    refused(blend(out=None, u8=None), b"ifx_vit_tile_blend", b"both outputs are null")
    refused(blend(batch=0), b"ifx_vit_tile_blend", b"empty output (0 x 9 x 56 x 40)")
    refused(blend(W=0), b"ifx_vit_tile_blend", b"empty output")
    refused(blend(nh=0), b"ifx_vit_tile_blend", b"empty tile grid (2 x 0 x 2)")
    refused(blend(lt=0), b"ifx_vit_tile_blend", b"limits (0, 24, 24)")
    refused(blend(lw=-24), b"ifx_vit_tile_blend", b"limits (8, 24, -24)")
    refused(blend(eh=-8), b"ifx_vit_tile_blend", b"blend extents (0, -8, 8)")
    refused(blend(ew=32), b"ifx_vit_tile_blend", b"blend extent (0, 8, 32)", b"larger than its limit (8, 24, 24)")
    refused(blend(et=9), b"ifx_vit_tile_blend", b"larger than its limit")
    refused(blend(T=17), b"ifx_vit_tile_blend", b"t_out (17)", b"2 tiles of limit 8")
    refused(blend(T=1), b"ifx_vit_tile_blend", b"t_out (1)")
    refused(blend(H=80), b"ifx_vit_tile_blend", b"h_out (80)", b"3 tiles of limit 24")
    refused(blend(W=56), b"ifx_vit_tile_blend", b"w_out (56)", b"2 tiles of limit 24")
    refused(blend(table=C.c_void_p(4100)), b"ifx_vit_tile_blend", b"table", b"8-byte")
    refused(blend(W=36), b"ifx_vit_tile_blend", b"vec_x", b"w_out (36)", b"multiples of 8")
    refused(blend(ew=4), b"ifx_vit_tile_blend", b"vec_x", b"blend_w (4)")
    refused(blend(lw=20, W=40), b"ifx_vit_tile_blend", b"vec_x", b"limit_w (20)")
    refused(blend(arena=P8), b"ifx_vit_tile_blend", b"16-byte")
    refused(blend(out=P8), b"ifx_vit_tile_blend", b"16-byte")
    refused(blend(u8=C.c_void_p(4100)), b"ifx_vit_tile_blend", b"out_u8 8-byte")
    refused(blend(arena=P1, vec=0), b"ifx_vit_tile_blend", b"2-byte")
    refused(blend(out=P1, vec=0), b"ifx_vit_tile_blend", b"2-byte")
    refused(blend(T=70000, nt=10000), b"ifx_vit_tile_blend", b"launch too large", b"70000 frames")
    refused(blend(batch=30000), b"ifx_vit_tile_blend", b"launch too large", b"30000 x 3 planes")


def test_blend_table_weights_are_the_python_float_expressions_cast_to_fp32():
    """w1 = fp32(1.0 - p / e') with the subtraction in double: for extents that are no powers of two, `1.0f - p / e'` in fp32 and
    weights rounded to bf16 first both give other bits (1 - 3 / 10 on this torch)."""
    import struct
    from inferix_amd.magi.tiles import plan_blend_table, plan_tiles
    desc = plan_blend_table(plan_tiles((3, 14, 11), 8, 96, 96, 0.25, 0.0, 8, 4), 1)        # extent 24; the edge tile blends over 16
    nt, nh, nw = desc.grid
    base = nt * nh * nw + 2 * (nt + nh + nw) + nt + nt * desc.blends[0] + nh * desc.blends[1]
    words = desc.words[base:]
    assert len(words) == nw * 24 and all(w == 0 for w in words[:24]) and all(w == 0 for w in words[24 + 16:])
    for p in range(16):
        w1, w2 = struct.unpack("<ff", struct.pack("<q", words[24 + p]))
        assert w1 == torch.tensor(1 - p / 16, dtype=torch.float64).float().item() and w2 == torch.tensor(p / 16).item()
    h = desc.words[base - nh * 24:base][24:]                         # the second tile of the height axis: e' = 24
    got = [struct.unpack("<ff", struct.pack("<q", w)) for w in h]
    want32 = [(float(torch.tensor(1.0) - torch.tensor(float(p)) / 24), float(torch.tensor(float(p)) / 24)) for p in range(24)]
    want = [(torch.tensor(1 - p / 24, dtype=torch.float64).float().item(), torch.tensor(p / 24, dtype=torch.float64).float().item())
            for p in range(24)]
    assert got == want and got != want32, "fp32 arithmetic on the weights is distinguishable at extent 24"
    t = torch.tensor([0.140625], dtype=BF)
    assert (t * (1 - 3 / 10)).item() != (t * torch.tensor(1 - 3 / 10).to(BF)).item()       # torch applies the weight at fp32 precision


def test_tile_blend_wrapper_refuses_cpu_tensors_and_short_arenas():
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi.tiles import plan_blend_table, plan_tiles
    desc = plan_blend_table(plan_tiles((3, 7, 5), 8, 32, 32, 0.25, 0.0, 8, 4), 1)
    assert desc.frame_pitch == (8, 1) and desc.arena_elements == desc.offsets[-1] + 3 * 1 * 8 * 16
    table = desc.tensor("cpu")
    with pytest.raises(_hip.HipKernelError):
        ops.vit_tile_blend(torch.zeros(desc.arena_elements, dtype=BF), desc, table)
    with pytest.raises(AssertionError):
        ops.vit_tile_blend(torch.zeros(desc.arena_elements - 1, dtype=BF), desc, table)


def test_shim_paths_resolve():
    from inferix.models.magi.vae import ViTVAE
    from inferix.pipeline.magi.video_process import VaeHelper
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    from inferix_amd.magi.vae import VaeHelper as V2
    assert VaeHelper is V2 and hasattr(ViTVAE, "tiled_decode_3d") and ViTVAE is HipMagiVAEDecoder
    sig = inspect.signature(VaeHelper.decode).parameters
    assert list(sig) == ["chunk", "vae", "tile_sample_min_height", "tile_sample_min_width", "spatial_tile_overlap_factor",
                         "temporal_tile_overlap_factor", "tile_sample_min_length", "allow_spatial_tiling", "uint8_output", "parallel_group"]
    assert sig["allow_spatial_tiling"].default is True and sig["uint8_output"].default is True


def test_no_tiles_fixture_is_above_the_size_limit():
    golden = os.path.join(ROOT, "tests", "golden")
    files = sorted(f for f in os.listdir(golden) if f.startswith("magi_tiles_"))
    assert files == sorted(n + s for n in TU.CASES for s in (".npz", "_raw.npz"))
    for f in files:
        assert os.path.getsize(os.path.join(golden, f)) <= 1 << 20, f

"""CPU: the MAGI ViT-VAE encoder and tiled prefix-encode fixtures and the host side of the encoder: tests/golden/magi_vitenc_*.npz and
magi_enc_tiles_*.npz hold what the reference's own `ViTEncoder` and `TileProcessor.tiled_encode` computed on the CPU in bf16
(tools/gen_golden_magi_vit_encoder.py).  The first tests guard them against the restatements of tests/magi_vit_encoder_util.py; the
others fail without the encode plan, the three `ifx_vit_*` encoder entry points, their bindings, the shims and the encoder classes."""
import ctypes as C
import os
import re

import pytest
import torch

import magi_vit_encoder_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_encoder_restatement_reproduces_the_reference_fixture_bit_for_bit(name):
    cfg, wseed, inputs, stored = E.CASES[name]
    fx = E.load_fixture(name)
    assert int(fx["weight_seed"]) == wseed
    W = E.make_encoder_weights(cfg, wseed)
    for n, (xseed, shape) in enumerate(inputs):
        sfx = "" if n == 0 else str(n + 1)
        x = E.make_video(xseed, shape)
        assert int(fx["input_seed" + sfx]) == xseed and torch.equal(x, fx["x" + sfx])
        taps = {}
        out = E.encoder_forward(W, cfg, x, taps)
        assert out.dtype == BF and torch.equal(out, fx["out" + sfx]), (name, n)
        assert tuple(out.shape) == (shape[0], cfg.out_channels) + tuple(s // p for s, p in zip(shape[2:], cfg.patch))
        if stored and n == 0:
            for k in ["patch_rows", "embed", "normed"] + [f"{t}{i}" for i in range(cfg.depth) for t in ("block", "qkv", "attn")]:
                assert torch.equal(taps[k], fx[k]), (name, k)
    if name in E.FP32_CASES:
        out32 = E.encoder_forward(E.make_encoder_weights(cfg, wseed, dtype=torch.float32), cfg, fx["x"].float())
        ref32 = E.load_fixture(name + "_fp32")["out"]
        # float32 sums depend on how many threads torch splits them over, so this one is not pinned to the bit: 1e-5 in rel-L2 is some
        # hundred float32 roundings and 1/500 of the floor the stored evaluation is used for
        assert out32.dtype == torch.float32 and out32.shape == ref32.shape
        assert float((out32.double() - ref32.double()).norm() / ref32.double().norm()) < 1e-5, name
        floor = float((fx["out"].double() - ref32.double()).norm() / ref32.double().norm())
        assert 1e-3 < floor < 2e-2, floor          # the bf16 evaluation sits a bf16-sized distance from the float32 one, no more


def test_patch_embedding_rounds_once_and_the_gather_is_the_convolution_operand():
    """bf16 Conv3d == bf16(fp32 accumulate + bias): the rounding the HIP embedding reproduces with one GEMM; and the gathered rows times
    `weight.flatten(1)` are that convolution."""
    cfg, wseed, inputs, _ = E.CASES["magi_vitenc_b"]
    W = E.make_encoder_weights(cfg, wseed)
    x = E.make_video(*inputs[1])                                                  # 10 x 36 x 44: trailing pixels on every axis
    conv = torch.nn.functional.conv3d(x, W["patch_embed.proj.weight"], W["patch_embed.proj.bias"], stride=cfg.patch)
    rows = E.gather_patch_rows(x, cfg.patch)
    assert rows.shape == (1, 2 * 4 * 5, 768)
    once = (rows.float() @ W["patch_embed.proj.weight"].flatten(1).float().T + W["patch_embed.proj.bias"].float()).to(BF)
    got = conv.flatten(2).transpose(1, 2)
    assert float((once.float() - got.float()).abs().max()) <= 2.0 ** -7 * float(got.float().abs().max())       # summation order only
    assert float((once != got).float().mean()) < 0.02


@pytest.mark.parametrize("name", sorted(E.TILE_CASES))
def test_tiled_encode_restatement_reproduces_the_reference_fixture_bit_for_bit(name):
    shape, tile_px, fs, ft, vseed, grid, out_shape = E.TILE_CASES[name]
    fx = E.load_fixture(name)
    pixels = E.make_pixels(vseed, shape)
    assert torch.equal(pixels, fx["pixels"]) and fx["tile_sample_min"].tolist() == list(tile_px) and fx["overlap_factors"].tolist() == [fs, ft]
    W = E.make_encoder_weights(E.TINY, E.TILE_WEIGHT_SEED)
    out = E.tiled_encode(E.encode_mode(W, E.TINY), E.normalise_pixels(pixels), **E.tile_case_kwargs(name))
    assert out.dtype == BF and torch.equal(out, fx["out"]) and tuple(out.shape) == (shape[0], 4) + out_shape


@pytest.mark.parametrize("name", sorted(E.TILE_CASES))
def test_in_place_chain_of_the_recorded_raw_tiles_gives_the_fixture_and_the_decode_rule_does_not(name):
    fx = E.load_fixture(name)
    axes = E.tile_case_axes(name)
    raw = E.load_raw_latent_tiles(fx, axes)
    assert torch.equal(E.blend_latent_tiles(raw, axes), fx["out"])
    other = E.blend_latent_tiles(raw, axes, in_place=False)
    assert torch.equal(other, fx["out_raw_neighbours"]) and not torch.equal(other, fx["out"])
    if name == "magi_enc_tiles_a":
        assert int((other != fx["out"]).sum()) == 24


@pytest.mark.parametrize("name", sorted(E.TILE_CASES))
def test_encode_plan_reproduces_the_recorded_tiles_of_the_reference(name):
    from inferix_amd.magi import tiles
    shape, tile_px, fs, ft, vseed, grid, out_shape = E.TILE_CASES[name]
    fx = E.load_fixture(name)
    plan = tiles.plan_encode_tiles(shape, tile_px[0], tile_px[1], tile_px[2], fs, ft, 8, 4)
    assert plan.grid == grid and plan.out_shape == out_shape
    axes = E.tile_case_axes(name)
    assert tuple(a.blend for a in plan.axes) == tuple(a.extent for a in axes) and tuple(a.limit for a in plan.axes) == tuple(a.limit for a in axes)
    called = [tuple(r) for r in fx["encode_shapes"].tolist()]
    assert len(called) == len(plan.tiles)
    for k, idx in enumerate(plan.tiles):
        assert (shape[0], 3) + plan.latent_shape(idx) == called[k], (name, idx)                     # the pixel shape `encode` was called with
        assert (shape[0], 4) + plan.decoded_shape(idx) == tuple(fx[f"tile_{k}"].shape), (name, idx)   # the latent shape it gave back
    if name == "magi_enc_tiles_a":
        assert len(plan.groups()) == 8
        assert plan.axes[1].extents == (4, 4, 1) and plan.axes[2].extents == (4, 2) and plan.axes[0].extents == (2, 1)


def test_encode_plan_at_the_prefix_video_geometry_and_its_refusals():
    from inferix_amd.magi import tiles
    plan = tiles.plan_encode_tiles((32, 720, 1280), 12, 256, 256, 0.25, 0, 8, 4)      # 32 frames at fps 24: tiles of fps // 2 frames
    assert plan.grid == (3, 4, 7) and plan.out_shape == (8, 90, 160)
    assert plan.axes[0].extents == (3, 3, 2) and plan.axes[1].extents == (32, 32, 32, 18) and plan.axes[1].blend == 8 and plan.axes[1].limit == 24
    one = tiles.plan_encode_tiles((1, 720, 1280), 12, 256, 256, 0.25, 0, 8, 4)        # an image: one frame -> one latent frame
    assert one.grid == (1, 4, 7) and one.out_shape == (1, 90, 160)
    with pytest.raises(NotImplementedError, match="does not line up"):
        tiles.plan_encode_tiles((32, 64, 64), 12, 40, 40, 0.25, 0, 8, 4)               # stride 30 px, limit 4 latents = 32 px
    with pytest.raises(ValueError, match="less than one patch"):
        tiles.plan_encode_tiles((10, 32, 32), 8, 32, 32, 0.25, 0, 8, 4)                # second temporal tile: 2 frames
    with pytest.raises(ValueError, match="less than one patch"):
        tiles.plan_encode_tiles((8, 50, 32), 8, 32, 32, 0.25, 0, 8, 4)                 # third tile of the height: 2 px
    desc = tiles.plan_latent_blend_table(plan, 16)
    assert desc.grid == (3, 4, 7) and desc.blends == (0, 8, 8) and len(desc.diagonal_max) == 3 + 4 + 7 - 2
    ids = list(desc.words[-84:])
    assert sorted(ids) == list(range(84)) and ids[0] == 0 and ids[-1] == 83
    assert desc.arena_elements == 16 * sum(a * b * c for a in (3, 3, 2) for b in (32, 32, 32, 18) for c in (32,) * 6 + (16,))


def test_latent_blend_table_weights_are_the_python_float_expressions_cast_to_fp32():
    import struct
    from inferix_amd.magi import tiles
    desc = tiles.latent_blend_table(4, [(2, 2), (4, 4, 1), (4, 2)], (1, 3, 1))
    nt, nh, nw = desc.grid
    at = 12 + 2 + 3 + 2 + nt * 1                                 # offsets, extents, the temporal weights
    words = desc.words[at:at + nh * 3]
    for k in range(nh):
        e = min((4, 4, 1)[k - 1], (4, 4, 1)[k], 3) if k else 0
        for p in range(3):
            w1, w2 = struct.unpack("<ff", struct.pack("<q", words[k * 3 + p]))
            want = (struct.unpack("<f", struct.pack("<f", 1 - p / e))[0], struct.unpack("<f", struct.pack("<f", p / e))[0]) if p < e else (0.0, 0.0)
            assert (w1, w2) == want, (k, p)


def test_encoder_exports_are_declared_bound_and_exported_without_an_abi_bump():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    lib = _hip.load()
    _vp, _i32, _f32, _i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64
    want = {"ifx_vit_patch_rows": [_vp, _i32, _vp, _vp, _vp, _i32, _vp] + [_i32] * 8 + [_vp],
            "ifx_vit_latent_head": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64] + [_i32] * 7 + [_f32, _vp],
            "ifx_vit_latent_blend": [_vp, _i64, _vp, _vp] + [_i32] * 7 + [_vp]}
    for name, args in want.items():
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(args), name
        assert _hip.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name) is not None
    assert (lib.ifx_version() >> 8) & 255 == 7 == _hip.ABI_MINOR and re.search(r"#define IFX_ABI_MINOR 7\b", hdr)


def test_encoder_argument_validation_without_gpu():
    """Every argument check of the three entry points answers before any launch (dummy aligned pointers, no GPU): code and message."""
    from inferix_amd import _hip
    lib = _hip.load()
    P, P2 = C.c_void_p(4096), C.c_void_p(4098)
    EINVAL, EUNSUP = -1, -3
    i64 = lambda *v: (C.c_int64 * len(v))(*v)

    def refused(rc, *parts, code=EINVAL):
        msg = lib.ifx_last_error()
        assert rc == code and all(p in msg for p in parts), (rc, msg)

    # (video, is_uint8, strides, dims, tiles, n_tiles, rows, ld, cls_tokens, patch_t, patch_h, patch_w, lat_t, lat_h, lat_w, stream)
    dims, strides, tile = i64(1, 3, 8, 32, 32), i64(24576, 8192, 1024, 32, 1), i64(0, 0, 0, 8, 32, 32)
    rows = lambda video=P, u8=0, strides=strides, dims=dims, tiles=tile, n=1, out=P, ld=768, cls=1, p=(4, 8, 8), lat=(2, 4, 4): \
        lib.ifx_vit_patch_rows(video, u8, strides, dims, tiles, n, out, ld, cls, *p, *lat, None)
    for null in ("video", "strides", "dims", "tiles", "out"):
        refused(rows(**{null: None}), b"ifx_vit_patch_rows", b"null")
    refused(rows(p=(0, 8, 8)), b"ifx_vit_patch_rows", b"bad patch 0 x 8 x 8")
    refused(rows(n=0), b"ifx_vit_patch_rows", b"n_tiles (0)")
    refused(rows(cls=-1), b"ifx_vit_patch_rows", b"cls_tokens (-1)")
    refused(rows(lat=(0, 4, 4)), b"ifx_vit_patch_rows", b"smaller than one patch")
    refused(rows(dims=i64(1, 4, 8, 32, 32)), b"ifx_vit_patch_rows", b"video dims [1, 4, 8, 32, 32]")
    refused(rows(strides=i64(24576, 8192, -1024, 32, 1)), b"ifx_vit_patch_rows", b"stride 2 is negative")
    refused(rows(ld=760), b"ifx_vit_patch_rows", b"768 elements", b"ld (760)")
    refused(rows(video=C.c_void_p(4097)), b"ifx_vit_patch_rows", b"2-byte aligned")
    refused(rows(tiles=i64(0, 0, 8, 8, 32, 32)), b"ifx_vit_patch_rows", b"tile 0 axis 2", b"outside the video (32)")
    refused(rows(tiles=i64(0, 0, 0, 3, 32, 32), lat=(1, 4, 4)), b"ifx_vit_patch_rows", b"tile 0 axis 0", b"extent 3 is smaller than one patch (4)")
    refused(rows(tiles=i64(0, 0, 0, 8, 32, 7), lat=(2, 4, 1)), b"ifx_vit_patch_rows", b"tile 0 axis 2", b"extent 7 is smaller than one patch (8)")
    refused(rows(tiles=i64(0, 0, 0, 8, 32, 24)), b"ifx_vit_patch_rows", b"tile 0 axis 2", b"extent 24 / patch 8", b"latent extent 4")
    refused(rows(tiles=i64(0, 0, 0, 8, 32, 32, 0, 8, 0, 8, 16, 32), n=2), b"ifx_vit_patch_rows", b"tile 1 axis 1", b"extent 16 / patch 8")

    # (x, ldx, gamma, beta, weight, bias, out, out_batch_stride, batch, rows_per_tile, cls_tokens, dim, channels, store, norm_code, eps, stream)
    head = lambda x=P, ldx=256, g=P, b=P, w=P, bias=P, out=P, stride=8 * 32, batch=1, rpt=33, cls=1, dim=256, ch=8, store=8: \
        lib.ifx_vit_latent_head(x, ldx, g, b, w, bias, out, stride, batch, rpt, cls, dim, ch, store, 0, 1e-5, None)
    for null in ("x", "g", "b", "w", "bias", "out"):
        refused(head(**{null: None}), b"ifx_vit_latent_head", b"null")
    refused(head(batch=0), b"ifx_vit_latent_head", b"batch (0)")
    refused(head(cls=33), b"ifx_vit_latent_head", b"cls_tokens (33)")
    refused(head(dim=2048, ldx=2048), b"ifx_vit_latent_head", b"dim 2048 x channels 8 not built", code=EUNSUP)
    refused(head(dim=252, ldx=256), b"ifx_vit_latent_head", b"dim 252 x channels 8 not built", code=EUNSUP)
    refused(head(ch=64, store=64), b"ifx_vit_latent_head", b"dim 256 x channels 64 not built", code=EUNSUP)
    refused(head(store=9), b"ifx_vit_latent_head", b"store_channels (9)")
    refused(head(store=0), b"ifx_vit_latent_head", b"store_channels (0)")
    refused(head(ldx=252), b"ifx_vit_latent_head", b"ldx (252)")
    refused(head(ldx=248), b"ifx_vit_latent_head", b"ldx (248)", b"dim (256)")
    refused(head(stride=255), b"ifx_vit_latent_head", b"out_batch_stride (255)", b"8 channels x 32 tokens")
    refused(head(x=C.c_void_p(4104)), b"ifx_vit_latent_head", b"16-byte")
    refused(head(w=C.c_void_p(4104)), b"ifx_vit_latent_head", b"16-byte")

    # (arena, arena_elements, table, max_tile_elements, planes, tiles_t, tiles_h, tiles_w, blend_t, blend_h, blend_w, stream)
    big = i64(512, 512, 512, 512, 512)                                # one per anti-diagonal: 2 + 3 + 2 - 2
    mix = lambda arena=P, n=4096, table=P, big=big, planes=4, grid=(2, 3, 2), e=(0, 1, 1): \
        lib.ifx_vit_latent_blend(arena, n, table, big, planes, *grid, *e, None)
    for null in ("arena", "table", "big"):
        refused(mix(**{null: None}), b"ifx_vit_latent_blend", b"null")
    refused(mix(n=0), b"ifx_vit_latent_blend", b"arena_elements (0)")
    refused(mix(planes=0), b"ifx_vit_latent_blend", b"planes (0)")
    refused(mix(grid=(0, 3, 2)), b"ifx_vit_latent_blend", b"tile grid 0 x 3 x 2")
    refused(mix(grid=(64, 64, 64)), b"ifx_vit_latent_blend", b"tile grid 64 x 64 x 64")
    refused(mix(e=(0, -1, 1)), b"ifx_vit_latent_blend", b"blend extents (0, -1, 1)")
    refused(mix(table=C.c_void_p(4100)), b"ifx_vit_latent_blend", b"8-byte")
    refused(mix(arena=C.c_void_p(4097)), b"ifx_vit_latent_blend", b"2-byte")
    refused(mix(big=i64(0, 512, 512, 512, 512)), b"ifx_vit_latent_blend", b"diagonal 0", b"max_tile_elements 0")
    assert mix(grid=(1, 1, 1), big=i64(512)) == 0                     # one tile: nothing to blend, no launch


def test_encoder_shim_paths_state_dict_rules_and_host_side_refusals():
    from inferix.models.magi.vae import ViTEncoder, ViTVAE
    from inferix.models.magi.vae.vae_module import ViTEncoder as E2
    from inferix.pipeline.magi.video_process import VaeHelper, encode_prefix_video
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi import vae as V
    assert ViTEncoder is E2 is V.HipViTEncoder and ViTVAE is V.HipMagiVAEDecoder
    assert VaeHelper is V.VaeHelper and encode_prefix_video is V.encode_prefix_video
    cfg = E.TINY
    enc = V.HipViTEncoder(**cfg.ctor_kwargs(), device="cpu")
    W = E.make_encoder_weights(cfg, 1)
    assert set(enc._expected()) == set(W), "the reference's state-dict keys"
    published = dict(video_size=256, video_length=16, patch_size=8, patch_length=4, embed_dim=1024, depth=24, num_heads=16, ln_in_attn=True,
                     conv_last_layer=True, use_final_proj=True, qkv_bias=True, z_chans=16)
    big = V.HipViTEncoder(**published, device="cpu")
    assert len(big._expected()) == 24 * 10 + 8 and big._expected()["patch_embed.proj.weight"] == (1024, 3, 4, 8, 8)
    assert big._expected()["last_layer.weight"] == (32, 1024) and big.latent_shape((10, 36, 44)) == (2, 4, 5)
    assert V.HipViTEncoder(**dict(published, double_z=False), device="cpu").out_channels == 16
    V.HipViTEncoder(**dict(published, conv_last_layer=False), device="cpu")          # ignored, as upstream
    with pytest.raises(NotImplementedError, match="use_rope"):
        V.HipViTEncoder(**dict(published, use_rope=True), device="cpu")
    with pytest.raises(NotImplementedError, match="head size"):
        V.HipViTEncoder(**dict(published, num_heads=8), device="cpu")
    with pytest.raises(NotImplementedError, match="qk_scale"):
        V.HipViTEncoder(**dict(published, qk_scale=0.1), device="cpu")
    with pytest.raises(NotImplementedError, match="norm_layer"):
        V.HipViTEncoder(**dict(published, norm_layer=torch.nn.RMSNorm), device="cpu")
    with pytest.raises(KeyError, match="patch_embed.proj.weight"):
        enc.load_state_dict({})
    enc.load_state_dict(W)
    with pytest.raises(_hip.HipKernelError):
        enc(torch.zeros(1, 3, 8, 32, 32, dtype=BF))

    # the vae: no encoder until encoder weights are loaded; then every encoder key is required
    import magi_vit_util as U
    DW = {"decoder." + k: v for k, v in U.make_weights(cfg, 2).items()}
    vae = V.HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cpu")
    assert vae.encoder is None
    for call in (lambda: vae.encode(None), lambda: vae.tiled_encode_3d(None)):
        with pytest.raises(NotImplementedError, match="encoder"):
            call()
    vae.load_state_dict(DW | {"encoder.proj_in.weight": torch.zeros(1), "encoder.norm.weight": torch.zeros(256)})
    assert vae.encoder is None and set(vae.state_dict()) == set(DW)
    EW = {"encoder." + k: v for k, v in W.items()}
    missing = dict(EW)
    del missing["encoder.last_layer.bias"]
    with pytest.raises(KeyError, match="encoder.last_layer.bias"):
        vae.load_state_dict(DW | missing)
    vae.load_state_dict(DW | EW)
    assert isinstance(vae.encoder, V.HipViTEncoder) and set(vae.state_dict()) == set(DW) | set(EW)
    assert all(torch.equal(vae.state_dict()[k], v) for k, v in EW.items())
    with pytest.raises(NotImplementedError, match="parallel_group"):
        vae.tiled_encode_3d(torch.zeros(1, 3, 8, 32, 32, dtype=BF), parallel_group=object())
    with pytest.raises(_hip.HipKernelError):
        vae.tiled_encode_3d(torch.zeros(1, 3, 8, 32, 32, dtype=BF))
    with pytest.raises(_hip.HipKernelError):
        vae.encode(torch.zeros(1, 3, 8, 32, 32, dtype=BF))
    for call in (lambda: ops.vit_patch_rows(torch.zeros(1, 3, 8, 32, 32, dtype=BF), [(0, 0, 0, 8, 32, 32)], (2, 4, 4), (4, 8, 8), cls_tokens=1),
                 lambda: ops.vit_latent_head(torch.zeros(33, 256, dtype=BF), torch.zeros(256, dtype=BF), torch.zeros(256, dtype=BF),
                                             torch.zeros(8, 256, dtype=BF), torch.zeros(8, dtype=BF), batch=1, cls_tokens=1, latent=(2, 4, 4))):
        with pytest.raises(_hip.HipKernelError):
            call()
    with pytest.raises(TypeError, match="uint8"):
        ops.vit_patch_rows(torch.zeros(1, 3, 8, 32, 32), [(0, 0, 0, 8, 32, 32)], (2, 4, 4), (4, 8, 8), cls_tokens=1)


def test_encode_prefix_video_plumbing_on_a_stub_vae(monkeypatch):
    """THWC -> NCTHW, tiles of fps // 2 frames and 256 px at overlap 0.25 with spatial tiling, the result times scale_factor."""
    from inferix_amd.magi import vae as V
    seen = {}

    class Stub(V.HipMagiVAEDecoder):
        def __init__(self):
            self.decoder = type("D", (), {"device": torch.device("cpu")})()

        def tiled_encode_3d(self, x, **kw):
            seen.update(kw, shape=tuple(x.shape), dtype=x.dtype, first=x[0, :, 2, 3, 4].clone())
            return torch.full((1, 4, 2, 3, 5), 2.0, dtype=BF)

    frames = torch.arange(9 * 24 * 40 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(9, 24, 40, 3)
    out = V.encode_prefix_video(frames, 24, Stub(), 0.5, parallel_group=None)
    assert seen["shape"] == (1, 3, 9, 24, 40) and seen["dtype"] == torch.uint8 and torch.equal(seen["first"], frames[2, 3, 4])
    assert seen["tile_sample_min_length"] == 12 and seen["tile_sample_min_height"] == seen["tile_sample_min_width"] == 256
    assert seen["spatial_tile_overlap_factor"] == 0.25 and seen["temporal_tile_overlap_factor"] == 0 and seen["allow_spatial_tiling"] is True
    assert seen["parallel_group"] is None and "deterministic" not in seen                      # the default: every tile the mode
    assert out.dtype == BF and torch.equal(out, torch.full((1, 4, 2, 3, 5), 1.0, dtype=BF))
    assert V.encode_prefix_video(None, 24, Stub(), 0.5) is None
    V.VaeHelper.encode(frames.permute(3, 0, 1, 2).unsqueeze(0).float(), Stub())                # float pixels: normalised here, to bf16
    assert seen["dtype"] == BF and float(seen["first"][0]) == float(((frames[2, 3, 4, 0].float() / 127.5) - 1.0).bfloat16())
    with pytest.raises(TypeError):
        V.VaeHelper.encode(frames.permute(3, 0, 1, 2).unsqueeze(0), object())


def test_no_encoder_fixture_is_above_the_size_limit():
    golden = os.path.join(ROOT, "tests", "golden")
    files = [f for f in os.listdir(golden) if f.startswith(("magi_vitenc_", "magi_enc_tiles_"))]
    assert len(files) == len(E.CASES) + len(E.FP32_CASES) + len(E.TILE_CASES)
    for f in files:
        assert os.path.getsize(os.path.join(golden, f)) <= 1 << 20, f

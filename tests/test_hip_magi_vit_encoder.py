"""GPU: the MAGI ViT-VAE encoder kernels (ifx_vit_patch_rows, ifx_vit_latent_head, ifx_vit_latent_blend), `HipViTEncoder` and the tiled
prefix-video encode of `HipMagiVAEDecoder` (inferix_amd/magi/vae.py) against the reference-generated fixtures tests/golden/magi_vitenc_*.npz
and magi_enc_tiles_*.npz.  The gather and the blend chain are bit-exact; the stages are teacher-forced under the bars of
tests/test_hip_magi_vae.py; end to end the measured-noise rule of that file applies: the float32 evaluation is the exact answer, the
reference's own bf16 result sits `floor` (rel-L2) from it, the HIP result must be within 1.25 x floor of the exact answer and within
2 x floor of the reference's.  Fixtures and seeds only."""
import dataclasses
import functools
from types import SimpleNamespace

import pytest
import torch

import magi_vit_encoder_util as E
import magi_vit_util as U
from util import assert_bf16_parity, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PATCH = (4, 8, 8)
SENTINEL = 1024.0
# the bar of a stage fed the reference's own input, as tests/test_hip_magi_vae.py states it: every element within 2 bf16 ULP at
# max(|ref|, tensor RMS), rel-L2 <= 3e-3, at most 0.2 of the elements differing at all (0.4 behind an attention)
STAGE = dict(max_ulp=2, floor=1.0, rel=3e-3, max_mismatch_frac=0.2)


@functools.lru_cache(maxsize=None)
def _case(name):
    from inferix_amd.magi.vae import HipViTEncoder
    cfg, wseed, inputs, stored = E.CASES[name]
    W = E.make_encoder_weights(cfg, wseed)
    enc = HipViTEncoder(**cfg.ctor_kwargs(), device="cuda:0")
    enc.load_state_dict(W)
    return cfg, W, enc, E.load_fixture(name)


@functools.lru_cache(maxsize=None)
def _floor(name, sfx=""):
    """(float32 evaluation, rel-L2 of the reference's bf16 moments from it, the same for the mean half).  Stored for (a) and (d); for
    the other cases the same restatement evaluates it here, once."""
    cfg, wseed, inputs, stored = E.CASES[name]
    fx = E.load_fixture(name)
    if name in E.FP32_CASES and not sfx:
        exact = E.load_fixture(name + "_fp32")["out"]
    else:
        exact = E.encoder_forward(E.make_encoder_weights(cfg, wseed, dtype=torch.float32), cfg, fx["x" + sfx].float())
    ref, z = fx["out" + sfx], cfg.z_chans
    return exact, rel_l2(ref, exact), rel_l2(ref[:, :z], exact[:, :z])


@functools.lru_cache(maxsize=None)
def _tiny_vae():
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    W = E.make_encoder_weights(E.TINY, E.TILE_WEIGHT_SEED)
    sd = {"decoder." + k: v for k, v in U.make_weights(E.TINY, 4100).items()} | {"encoder." + k: v for k, v in W.items()}
    vae = HipMagiVAEDecoder(E.TINY.ctor_kwargs(), device="cuda:0")
    vae.load_state_dict(sd)
    return vae, W


# ---- ifx_vit_patch_rows ---------------------------------------------------------------------------------------------------------------
def _expect_rows(video, tiles, cls=1):
    """The torch gather of every (tile, sample), class rows marked with the sentinel."""
    out = []
    for t0, h0, w0, Te, He, We in tiles:
        rows = E.gather_patch_rows(video[:, :, t0:t0 + Te, h0:h0 + He, w0:w0 + We], PATCH)
        out.append(torch.cat((torch.full((rows.shape[0], cls, rows.shape[2]), SENTINEL, dtype=rows.dtype), rows), dim=1))
    return torch.cat(out).flatten(0, 1)


def _run_rows(video_gpu, tiles, cls=1):
    """ifx_vit_patch_rows into a sentinel-filled buffer with one canary row behind it -> (rows, canary row)."""
    from inferix_amd import hip_ops as ops
    latent = tuple(e // p for e, p in zip(tiles[0][3:], PATCH))
    n = len(tiles) * video_gpu.shape[0] * (cls + latent[0] * latent[1] * latent[2])
    buf = torch.full((n + 1, 768), SENTINEL, dtype=BF, device="cuda:0")
    ops.vit_patch_rows(video_gpu, tiles, latent, PATCH, cls_tokens=cls, out=buf[:n])
    torch.cuda.synchronize()
    return buf[:n].cpu(), buf[n].cpu()


def _check_rows(video_cpu_as_bf16, video_gpu, tiles, what):
    got, canary = _run_rows(video_gpu, tiles)
    want = _expect_rows(video_cpu_as_bf16, tiles)
    assert got.shape == want.shape and torch.equal(got, want), what
    assert torch.all(canary == SENTINEL), f"{what}: the row behind the buffer was written"


def test_patch_rows_bf16_remainder_and_two_tiles_bit_exact():
    x = E.make_video(51, (2, 3, 10, 36, 48))                 # rows of 48 pixels: every row start is 16-byte aligned
    xg = x.cuda()
    _check_rows(x, xg, [(0, 0, 0, 8, 32, 32)], "bf16, one tile, 16-byte path")
    _check_rows(x, xg, [(0, 0, 0, 10, 36, 44)], "bf16, 16-byte path, remainder: 10 x 36 x 44 floors to (2, 4, 5)")
    _check_rows(x, xg, [(0, 0, 0, 8, 32, 32), (2, 4, 16, 8, 32, 32)], "bf16, two tiles, origins aligned to 8 along w")
    _check_rows(x, xg, [(0, 0, 0, 8, 32, 32), (1, 3, 5, 9, 33, 39)], "bf16, two tiles, an odd w origin: one element per lane")
    _check_rows(x, xg, [(6, 28, 40, 4, 8, 8)], "bf16, a single-patch tile in the far corner")
    odd = E.make_video(56, (1, 3, 10, 36, 44))               # the remainder case as a whole video: rows of 44 pixels, one element per lane
    _check_rows(odd, odd.cuda(), [(0, 0, 0, 10, 36, 44)], "bf16, whole 10 x 36 x 44 video")


def test_patch_rows_all_uint8_values():
    """Every uint8 value through both paths: bf16(fp32(v) / 127.5 - 1.0), what `VaeHelper.encode` computes with torch."""
    g = torch.Generator().manual_seed(52)
    px = torch.cat((torch.arange(256), torch.randint(0, 256, (3 * 8 * 32 * 40 - 256,), generator=g))).to(torch.uint8).view(1, 3, 8, 32, 40)
    want_video = E.normalise_pixels(px)
    assert len(set(want_video.flatten().tolist())) <= 256
    _check_rows(want_video, px.cuda(), [(0, 0, 0, 8, 32, 32)], "uint8, 8-byte path")
    _check_rows(want_video, px.cuda(), [(0, 0, 0, 8, 32, 40)], "uint8, whole video")
    _check_rows(want_video, px.cuda(), [(0, 0, 3, 8, 32, 32)], "uint8, odd w origin: one element per lane")


def test_patch_rows_window_of_a_poisoned_video_and_the_single_frame_expand():
    big = torch.full((1, 3, 12, 48, 56), float("nan"), dtype=BF)
    x = E.make_video(53, (1, 3, 8, 32, 40))
    big[:, :, 2:10, 8:40, 8:48] = x
    window = big.cuda()[:, :, 2:10, 8:40, 8:48]
    assert not window.is_contiguous()
    got, canary = _run_rows(window, [(0, 0, 0, 8, 32, 40)])
    assert torch.isfinite(got.float()).all(), "a NaN of the surrounding video reached the rows"
    assert torch.equal(got, _expect_rows(x, [(0, 0, 0, 8, 32, 40)])) and torch.all(canary == SENTINEL)
    # a tile inside the window, trailing pixels of the tile (and the NaNs behind the window) never read
    got, _ = _run_rows(window, [(4, 8, 16, 4, 24, 24)])
    assert torch.equal(got, _expect_rows(x, [(4, 8, 16, 4, 24, 24)]))
    # T == 1: `x.expand(-1, -1, 4, -1, -1)` is a T stride of 0
    one = E.make_video(54, (2, 3, 1, 16, 24))
    exp = one.cuda().expand(-1, -1, 4, -1, -1)
    assert exp.stride(2) == 0
    _check_rows(one.expand(-1, -1, 4, -1, -1), exp, [(0, 0, 0, 4, 16, 24)], "stride-0 expand")


# ---- ifx_vit_latent_head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_code", [False, True])
def test_latent_head_on_fixture_rows(norm_code):
    """The rows the reference's last block produced (fixture (a)) through the restated chain of :542-557, without and with norm_code."""
    from inferix_amd import hip_ops as ops
    cfg, W, enc, fx = _case("magi_vitenc_a")
    cfg = dataclasses.replace(cfg, norm_code=norm_code)
    h = fx[f"block{cfg.depth - 1}"]
    want = E.latent_head(W, cfg, h, (2, 4, 4))
    if not norm_code:
        assert torch.equal(want, fx["out"])
    w = enc.w
    got = ops.vit_latent_head(h.cuda().view(33, 256), w["norm.weight"], w["norm.bias"], w["last_layer.weight"], w["last_layer.bias"], batch=1,
                              cls_tokens=1, latent=(2, 4, 4), norm_code=norm_code)
    assert_bf16_parity(got, want, **STAGE, what=f"latent head, norm_code={norm_code}", report=True)
    mean = ops.vit_latent_head(h.cuda().view(33, 256), w["norm.weight"], w["norm.bias"], w["last_layer.weight"], w["last_layer.bias"], batch=1,
                               cls_tokens=1, latent=(2, 4, 4), norm_code=norm_code, store_channels=4)
    assert torch.equal(mean, got[:, :4]), "store_channels keeps the leading channels"


def test_latent_head_wide_rows_into_an_arena_slot_with_canaries():
    """Width 1024 with 32 channels (64 KiB of weight in LDS), 120 tiles of 2 x 3 x 3 + class row = 2280 rows, more than the launch's
    workgroups hold at once, so they walk; the output is a window of a larger arena with its own batch stride: nothing outside the
    slots is written, and the class rows contribute nothing."""
    from inferix_amd import hip_ops as ops
    cfg = E.CASES["magi_vitenc_c"][0]
    W = E.make_encoder_weights(cfg, 5200)
    g = torch.Generator().manual_seed(55)
    latent, B = (2, 3, 3), 120
    h = (torch.randn(B, 19, 1024, generator=g) * 1.5).to(BF)
    h[:, 0] = float("nan")                                    # class rows: skipped, not multiplied
    want = E.latent_head(W, cfg, h, latent)
    dev = {k: W[k].cuda() for k in ("norm.weight", "norm.bias", "last_layer.weight", "last_layer.bias")}
    tokens, stride = 18, 32 * 18 + 40
    arena = torch.full((8 + B * stride,), SENTINEL, dtype=BF, device="cuda:0")
    slot = arena[8:].view(B, stride)[:, :32 * tokens].view(B, 32, *latent)
    ops.vit_latent_head(h.cuda().view(B * 19, 1024), dev["norm.weight"], dev["norm.bias"], dev["last_layer.weight"], dev["last_layer.bias"],
                        batch=B, cls_tokens=1, latent=latent, norm_code=True, out=slot)
    assert_bf16_parity(slot, want, **STAGE, what="latent head 1024 x 32, norm_code", report=True)
    rest = arena.clone()
    rest[8:].view(B, stride)[:, :32 * tokens] = SENTINEL
    assert torch.all(rest == SENTINEL), "written outside the slots"
    norms = slot.float().norm(dim=1)
    assert float((norms - 1).abs().max()) < 2e-2               # norm_code: unit L2 norm over the channels, to bf16 rounding


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["magi_vitenc_a", "magi_vitenc_b"])
def test_encoder_stages_teacher_forced(name):
    """Every stage fed the reference's own input to it: the gather, the embedding; per block the qkv projection + head prep, the
    attention, the rest of the block; the head."""
    cfg, W, enc, fx = _case(name)
    B, N, D = fx["embed"].shape
    rows = lambda t: t.cuda().reshape(B * N, -1)
    x = fx["x"].cuda()
    pr, batch, latent = enc.patch_rows(x)
    assert batch == B and latent == tuple(fx["out"].shape[2:])
    assert torch.equal(pr.view(B, N, -1)[:, 1:].cpu(), fx["patch_rows"]), f"{name}: patch rows"
    assert_bf16_parity(enc.embed(x), fx["embed"], max_ulp=1, floor=1.0, what=f"{name} embed", report=True)
    h = fx["embed"]
    for i in range(cfg.depth):
        qkv, attn, out = fx[f"qkv{i}"], fx[f"attn{i}"], fx[f"block{i}"]
        assert_bf16_parity(enc.attn_inputs(i, rows(h), B).view(B, N, 3 * D), qkv, **STAGE, what=f"{name} block {i} qkv + head prep", report=True)
        assert_bf16_parity(enc.attention(rows(qkv), B).view(B, N, D), attn, **dict(STAGE, max_mismatch_frac=0.4),
                           what=f"{name} block {i} attention", report=True)
        assert_bf16_parity(enc.block_tail(i, rows(h), rows(attn)).view(B, N, D), out, **STAGE, what=f"{name} block {i} tail", report=True)
        h = out
    assert_bf16_parity(enc.head(rows(h), B, latent), fx["out"], **STAGE, what=f"{name} head", report=True)


@pytest.mark.parametrize("name,sfx", [("magi_vitenc_a", ""), ("magi_vitenc_b", ""), ("magi_vitenc_b", "2"), ("magi_vitenc_c", ""),
                                      ("magi_vitenc_d", "")])
def test_encoder_end_to_end_measured_noise(name, sfx):
    cfg, W, enc, fx = _case(name)
    exact, floor, floor_mean = _floor(name, sfx)
    out = enc(fx["x" + sfx].cuda()).cpu()
    ref, z = fx["out" + sfx], cfg.z_chans
    assert out.shape == ref.shape and out.dtype == BF and torch.isfinite(out.float()).all()
    for what, o, r, e, fl in (("moments", out, ref, exact, floor), ("mean", out[:, :z], ref[:, :z], exact[:, :z], floor_mean)):
        err_exact, err_ref = rel_l2(o, e), rel_l2(o, r)
        line = (f"{name}{sfx} {what}: bf16 floor {fl:.3e}, HIP vs float32 {err_exact:.3e} (bound {1.25 * fl:.3e}), HIP vs reference "
                f"{err_ref:.3e} (bound {2 * fl:.3e})")
        print(line)
        assert err_exact <= 1.25 * fl and err_ref <= 2.0 * fl, line


def test_encoder_is_deterministic_batch_invariant_and_the_single_frame_rule():
    cfg, W, enc, fx = _case("magi_vitenc_a")
    vae, _ = _tiny_vae()
    x0 = fx["x"].cuda()
    x1 = E.make_video(77, (1, 3, 8, 32, 32)).cuda()
    a, b = enc(x0), enc(x0)
    assert torch.equal(a, b), "two calls differ"
    both = enc(torch.cat((x0, x1)))
    assert torch.equal(both[0:1], a) and torch.equal(both[1:2], enc(x1)), "batch 2 differs from two batch-1 calls"
    assert torch.equal(vae.encode(x0, sample_posterior=False), a[:, :4]), "the mode is the mean half"
    frame = E.make_video(78, (1, 3, 1, 40, 24)).cuda()
    one = vae.encode(frame, sample_posterior=False)
    full = vae.encoder(frame.expand(-1, -1, 4, -1, -1).contiguous())
    assert one.shape == (1, 4, 1, 5, 3) and torch.equal(one, full[:, :4, :1])
    # the sample: mean + exp(0.5 clamp(logvar)) * noise with the caller's generator
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    s = vae.encode(x0, generator=gen)
    mean, logvar = a[:, :4], a[:, 4:]
    noise = torch.randn(mean.shape, dtype=BF, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(5))
    assert s.dtype == BF and torch.equal(s, mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * noise)


# ---- the tile pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.TILE_CASES))
def test_blend_chain_on_the_recorded_raw_tiles_is_bit_identical(name):
    """ifx_vit_latent_blend fed the raw tile latents the reference's own `encode` calls returned: the reference's result bit for bit,
    corners included, and not the result of the decode-style blend against raw neighbours."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.magi import tiles
    from inferix_amd.magi.vae import assemble_encoded_tiles
    shape, tile_px, fs, ft, vseed, grid, out_shape = E.TILE_CASES[name]
    fx = E.load_fixture(name)
    plan = tiles.plan_encode_tiles(shape, tile_px[0], tile_px[1], tile_px[2], fs, ft, 8, 4)
    desc = tiles.plan_latent_blend_table(plan, shape[0] * 4)
    arena = torch.full((desc.arena_elements + 16,), SENTINEL, dtype=BF, device="cuda:0")
    for k, o in enumerate(desc.offsets):
        t = fx[f"tile_{k}"]
        arena[o:o + t.numel()] = t.cuda().flatten()
    ops.vit_latent_blend(arena[:desc.arena_elements], desc, desc.tensor("cuda:0"))
    out = assemble_encoded_tiles(arena, plan, desc.offsets, shape[0], 4).cpu()
    assert torch.equal(out, fx["out"]), f"{name}: {int((out != fx['out']).sum())} elements differ from the reference's chain"
    assert not torch.equal(out, fx["out_raw_neighbours"])
    assert torch.all(arena[desc.arena_elements:] == SENTINEL), "written behind the arena"


@pytest.mark.parametrize("name", sorted(E.TILE_CASES))
def test_tiled_encode_end_to_end(name):
    """`tiled_encode_3d` and `VaeHelper.encode` on the tile fixtures: the measured-noise rule against the reference's result, one tile
    per forward equal to the shape-batched run, uint8 pixels equal to the pre-normalised bf16 video."""
    from inferix_amd.magi.vae import VaeHelper
    vae, W = _tiny_vae()
    fx = E.load_fixture(name)
    kw = E.tile_case_kwargs(name)
    video = E.normalise_pixels(fx["pixels"])
    W32 = E.make_encoder_weights(E.TINY, E.TILE_WEIGHT_SEED, dtype=torch.float32)
    exact = E.tiled_encode(E.encode_mode(W32, E.TINY), video.float(), **kw)
    floor = rel_l2(fx["out"], exact)
    out = vae.tiled_encode_3d(video.cuda(), **kw)
    assert out.shape == fx["out"].shape and out.dtype == BF
    err_exact, err_ref = rel_l2(out.cpu(), exact), rel_l2(out.cpu(), fx["out"])
    line = (f"{name}: bf16 floor {floor:.3e}, HIP vs float32 {err_exact:.3e} (bound {1.25 * floor:.3e}), HIP vs reference {err_ref:.3e} "
            f"(bound {2 * floor:.3e})")
    print(line)
    assert err_exact <= 1.25 * floor and err_ref <= 2.0 * floor, line
    assert torch.equal(vae.tiled_encode_3d(video.cuda(), **kw, max_rows_per_forward=1), out), "one tile per forward differs"
    assert torch.equal(vae.tiled_encode_3d(fx["pixels"].cuda(), **kw), out), "uint8 pixels differ from the normalised bf16 video"
    assert torch.equal(VaeHelper.encode(fx["pixels"], vae, **kw), out), "VaeHelper.encode"


def test_tiled_encode_samples_when_not_deterministic():
    vae, W = _tiny_vae()
    fx = E.load_fixture("magi_enc_tiles_a")
    kw = E.tile_case_kwargs("magi_enc_tiles_a")
    px = fx["pixels"].cuda()
    mode = vae.tiled_encode_3d(px, **kw)
    g = lambda: torch.Generator(device="cuda:0").manual_seed(9)
    s0, s1 = vae.tiled_encode_3d(px, **kw, deterministic=False, generator=g()), vae.tiled_encode_3d(px, **kw, deterministic=False, generator=g())
    assert s0.shape == mode.shape and torch.equal(s0, s1) and not torch.equal(s0, mode) and torch.isfinite(s0.float()).all()


class _Recorder:
    def __init__(self):
        self.runtime_config = SimpleNamespace(clean_t=0.9999, noise2clean_kvrange=[5, 4, 3, 2], clean_chunk_kvrange=1, cfg_number=1)
        self.engine_config = SimpleNamespace(shortcut_mode="8,16,16", distill_nearly_clean_chunk_threshold=0.3)
        self.model_config = SimpleNamespace(patch_size=2)
        self.calls = []

    def forward_dispatcher(self, x, timestep, y, mask, kv_range, inference_params, **kw):
        self.calls.append((x.clone(), dict(kw)))
        return torch.ones_like(x)


def test_encode_prefix_video_hands_clean_latents_to_the_chunk_schedule():
    """A 2-chunk prefix clip (chunks of 2 latent frames: 16 frames) -> `[1, z, 4, H / 8, W / 8]` bf16 x scale_factor, which
    `ChunkSchedule.run(prefix_video=...)` takes: the extraction pass sees exactly these latents."""
    from inferix_amd.magi import schedule as S
    from inferix_amd.magi.vae import encode_prefix_video
    vae, W = _tiny_vae()
    frames = E.make_pixels(61, (16, 32, 48, 3)).cuda()                        # THWC, as the readers deliver it
    prefix = encode_prefix_video(frames, 16, vae, 0.5)                         # fps 16: tiles of 8 frames
    assert prefix.shape == (1, 4, 4, 4, 6) and prefix.dtype == BF and prefix.is_cuda
    plain = vae.tiled_encode_3d(frames.permute(3, 0, 1, 2).unsqueeze(0).contiguous(), tile_sample_min_length=8, allow_spatial_tiling=True)
    assert torch.equal(prefix, plain * 0.5)
    cw, chunks = 2, 4
    sch = S.ChunkSchedule(8, 4, chunks, cw, chunk_offset=2)
    x = torch.zeros(2, 4, chunks * cw, 4, 6, dtype=BF, device="cuda:0")
    y, masks = torch.zeros(2, chunks, 3, 8, device="cuda:0"), torch.ones(2, chunks, 3, device="cuda:0")
    m = _Recorder()
    sch.run(m, x, y, masks, inference_params=None, prefix_video=prefix, steps=[0])
    seen, kw = m.calls[0]
    assert kw["extract_prefix_video_feature"] and seen.dtype == BF and seen.shape == (2, 4, 4, 4, 6)
    assert torch.equal(seen[0:1], prefix) and torch.equal(seen[1:2], prefix)

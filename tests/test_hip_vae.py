"""GPU parity of the VAE decoder path: `ifx_conv3d_cl`, `ifx_rmsnorm_cl`, `ifx_softmax_rows` per op and
`HipWanVAEWrapper.decode_to_pixel` end to end against the CPU oracle and the reference-generated golden pixels."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")        # the on-device oracle of the 480p test: no exhaustive kernel search

import pytest
import torch
import torch.nn.functional as F

import vae_oracle as V
from conv_cases import NORM_DECODER_CASES, ref_conv
from fixture_io import golden, weights_checksum
from util import assert_bf16_parity, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


CASES = [
    # kt ks ups cin cout  h   w  t  residual
    (3, 3, 0, 32, 32, 8, 64, 1, False),
    (3, 3, 0, 96, 96, 13, 70, 2, True),
    (3, 3, 0, 64, 128, 9, 33, 3, False),
    (3, 3, 0, 192, 384, 5, 12, 2, True),
    (3, 3, 0, 96, 3, 17, 65, 2, False),
    (1, 3, 1, 64, 32, 6, 40, 2, False),
    (1, 3, 1, 192, 96, 7, 33, 3, False),
    (3, 1, 0, 64, 64, 8, 12, 3, False),
    (3, 1, 0, 128, 128, 11, 67, 2, False),
    (1, 1, 0, 32, 16, 8, 12, 3, False),
    (1, 1, 0, 64, 128, 10, 66, 2, False),
]


# the ping-pong kernel's shapes (3 x 3 spatial, cout % 96 == 0): 6 to 45 tiles (several tile rows, columns, channel tiles and frames per
# launch, ragged last rows and columns), up to 36 stages per tile, both layouts; and cout 3 / 24 on the same frames (lock-step kernel, 32
# tile).  With 45 tiles at most every workgroup runs ONE tile on any part with 48 compute units or more: a workgroup that runs several is
# test_hip_conv_edges.py::test_persistent_kernel_with_more_tiles_than_workgroups
CASES += [
    (3, 3, 0, 96, 96, 40, 150, 3, True),
    (3, 3, 0, 384, 192, 11, 70, 2, True),
    (3, 3, 0, 32, 96, 21, 130, 1, False),
    (1, 3, 1, 384, 192, 9, 40, 2, False),
    (1, 3, 0, 96, 96, 17, 64, 2, True),
    (3, 3, 0, 96, 3, 40, 150, 3, False),
    (3, 3, 0, 64, 24, 19, 70, 2, True),
]

# two choices of the launch plan that no decoder layer makes: the 128-channel tile with a ragged second tile (cout 160), and
# cout > 512 on 96-channel tiles, which the persistent kernel's 1 KiB bias copy in LDS rules out (the lock-step kernel under conv_variant 0)
CASES += [
    (3, 3, 0, 32, 160, 9, 33, 2, True),
    (1, 3, 0, 32, 576, 9, 70, 1, False),
]


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("kt,ks,ups,cin,cout,h,w,t,res", CASES)
def test_conv3d_cl_against_torch(ops, kt, ks, ups, cin, cout, h, w, t, res, planar):
    """`planar`: the input frames in the 32-channel-plane layout of the frame rings (ifx_conv3d_desc.in_planar) — the same bits."""
    g = torch.Generator().manual_seed(kt * 1000 + ks * 100 + cin + cout + h + w)
    n_in = t + kt - 1
    frames = rnd(g, n_in, h, w, cin)
    wt = rnd(g, cout, cin, kt, ks, ks, scale=(cin * kt * ks * ks) ** -0.5)
    b = rnd(g, cout, scale=0.1)
    ho, wo = (2 * h, 2 * w) if ups else (h, w)
    residual = rnd(g, t, ho, wo, cout) if res else None
    # physical slots: shuffled, with spare slots in between
    perm = torch.randperm(n_in + 2, generator=g)[:n_in].tolist()
    buf = torch.full((n_in + 2, h, w, cin), float("nan"), dtype=BF)
    for f, s in enumerate(perm):
        buf[s] = frames[f]
    out_slots = torch.randperm(t + 1, generator=g)[:t].tolist()
    y = torch.zeros(t + 1, ho, wo, cout, dtype=BF, device="cuda")
    from inferix_amd.vae import _repack_conv
    xin = ops.to_planar(buf.cuda()) if planar else buf.cuda()
    ops.conv3d_cl(xin, perm, _repack_conv(wt).cuda(), b.cuda(), kt=kt, ks=ks, y=y, out_slots=out_slots,
                  upsample=bool(ups), residual=residual.cuda() if res else None)
    ref = ref_conv(frames, wt, b, kt, ks, ups, residual)
    got = torch.stack([y[s] for s in out_slots]).cpu()
    assert_bf16_parity(got, ref, max_ulp=2 if res else 1, floor=1.0, what=f"conv kt{kt} ks{ks} ups{ups} {cin}->{cout}")
    untouched = [s for s in range(t + 1) if s not in out_slots]
    assert all(float(y[s].abs().max()) == 0.0 for s in untouched)
    if ks == 3 and cout % 96 == 0:
        # the lock-step kernel of round 1 on the same launch: the same K order and epilogue rounding, bit for bit
        y1 = torch.zeros_like(y)
        ops.set_option("conv_variant", 1)
        try:
            ops.conv3d_cl(xin, perm, _repack_conv(wt).cuda(), b.cuda(), kt=kt, ks=ks, y=y1, out_slots=out_slots,
                          upsample=bool(ups), residual=residual.cuda() if res else None)
        finally:
            ops.set_option("conv_variant", 0)
        assert torch.equal(y.view(torch.int16), y1.view(torch.int16)), "ping-pong and lock-step conv kernels differ"


def test_conv3d_cl_zero_history_is_causal_padding(ops):
    """in_slots < 0 = the zero frames in front of the stream (vae.py:26-34 without a cache)."""
    g = torch.Generator().manual_seed(5)
    h, w, cin, cout = 9, 20, 64, 64
    x = rnd(g, 2, h, w, cin)
    wt, b = rnd(g, cout, cin, 3, 3, 3, scale=(cin * 27) ** -0.5), rnd(g, cout, scale=0.1)
    from inferix_amd.vae import _repack_conv
    y = torch.empty(2, h, w, cout, dtype=BF, device="cuda")
    ops.conv3d_cl(x.cuda(), [-1, -1, 0, 1], _repack_conv(wt).cuda(), b.cuda(), kt=3, ks=3, y=y, out_slots=[0, 1])
    ref = V.causal_conv3d(x.permute(3, 0, 1, 2).unsqueeze(0), wt, b, None)[0].permute(1, 2, 3, 0)
    assert_bf16_parity(y.cpu(), ref, floor=1.0, what="zero history")
    # one cached frame: [zero, cached, new]
    ops.conv3d_cl(x.cuda(), [-1, 0, 1], _repack_conv(wt).cuda(), b.cuda(), kt=3, ks=3, y=y[:1], out_slots=[0])
    ref1 = V.causal_conv3d(x[1:2].permute(3, 0, 1, 2).unsqueeze(0), wt, b, x[0:1].permute(3, 0, 1, 2).unsqueeze(0))
    assert_bf16_parity(y[:1].cpu(), ref1[0].permute(1, 2, 3, 0), floor=1.0, what="one cached frame")


def test_conv3d_cl_argument_errors(ops):
    from inferix_amd import _hip
    x = torch.zeros(3, 8, 8, 64, dtype=BF, device="cuda")
    w = torch.zeros(27, 2, 32, 32, dtype=BF, device="cuda")
    y = torch.zeros(1, 8, 8, 32, dtype=BF, device="cuda")
    with pytest.raises(_hip.HipKernelError, match="temporal kernel"):
        d = _hip.Conv3dDesc(x.data_ptr(), 8 * 8 * 64, (C.c_int32 * 3)(0, 1, 2), 8, 8, 64, 0, w.data_ptr(), None, 2, 3, y.data_ptr(),
                            8 * 8 * 32, (C.c_int32 * 1)(0), 32, 1, None, x.data_ptr())
        _hip.check(_hip.load().ifx_conv3d_cl(C.byref(d), torch.cuda.current_stream().cuda_stream), "ifx_conv3d_cl")
    x48 = torch.zeros(3, 8, 8, 48, dtype=BF, device="cuda")
    with pytest.raises(AssertionError):
        ops.conv3d_cl(x48, [0, 1, 2], w, None, kt=3, ks=3, y=y, out_slots=[0])


@pytest.mark.parametrize("c,silu", NORM_DECODER_CASES)
def test_rmsnorm_cl(ops, c, silu):
    g = torch.Generator().manual_seed(c)
    x = rnd(g, 3, 7, 9, c, scale=3.0)
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(BF)
    y = torch.zeros(5, 7, 9, c, dtype=BF, device="cuda")
    ops.rmsnorm_cl(x.cuda(), gamma.cuda(), y, [4, 0, 2], silu=silu)
    ref = V.rms_norm(x, gamma, channel_dim=-1)
    if silu:
        ref = F.silu(ref)
    got = torch.stack([y[4], y[0], y[2]]).cpu()
    assert_bf16_parity(got, ref, max_ulp=2, floor=0.05, what=f"rmsnorm_cl c{c} silu{silu}")
    assert float(y[1].abs().max()) == 0.0 and float(y[3].abs().max()) == 0.0
    # the planar output layout (IFX_NORM_OUT_PLANAR): the same values, 32-channel planes
    yp = torch.zeros(5, c // 32, 7, 9, 32, dtype=BF, device="cuda")
    ops.rmsnorm_cl(x.cuda(), gamma.cuda(), yp, [4, 0, 2], silu=silu)
    assert torch.equal(yp.view(torch.int16), ops.to_planar(y).view(torch.int16))


@pytest.mark.parametrize("rows,cols", [(96, 96), (130, 250), (7, 6240), (1, 1), (5, 7), (3, 513), (9, 520)])
def test_softmax_rows(ops, rows, cols):
    g = torch.Generator().manual_seed(rows)
    ld = (cols + 63) // 64 * 64
    s = torch.zeros(rows, ld, dtype=BF)
    s[:, :cols] = rnd(g, rows, cols, scale=4.0)
    p = torch.zeros(rows, ld, dtype=BF, device="cuda")
    ops.softmax_rows(s.cuda()[:, :cols], 0.3, out=p[:, :cols])
    ref = torch.softmax(s[:, :cols].double() * 0.3, -1).to(BF)
    assert_bf16_parity(p[:, :cols].cpu(), ref, max_mismatch_frac=0.1, floor=0.0, what=f"softmax rows {rows}x{cols}", report=True)
    assert float(p[:, cols:].abs().max()) == 0.0 if ld > cols else True


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    g = golden("vae_decode.npz")
    cfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    W = V.make_decoder_params(cfg, int(g["seed"]))
    assert weights_checksum(W) == int(g["weights_checksum"])
    from inferix_amd.vae import HipWanVAEWrapper
    return g, cfg, W, HipWanVAEWrapper(W, dim=cfg.dim)


def test_decode_matches_reference_golden(tiny):
    g, cfg, W, vae = tiny
    got = vae.decode_to_pixel(g["latent"].cuda(), use_cache=True, chunk_size=1).cpu()
    ref = g["pixels"]
    assert got.shape == ref.shape and got.dtype == torch.float32
    r = rel_l2(got, ref)
    d = (got - ref).abs()
    print(f"decode vs reference golden: rel L2 {r:.3e}, max abs {float(d.max()):.3e}, mean abs {float(d.mean()):.3e}")
    # Tolerance: the network is 33 bf16 convs deep and every layer rounds to bf16 on both sides, so two correct bf16
    # evaluations differ by the accumulated rounding noise.  That noise is MEASURED here: the fp32 evaluation of the same
    # decoder (oracle, dtype float32) is the exact answer; the reference's own bf16 pixels sit `floor` away from it
    # (1.3e-2 rel L2 on this fixture).  The HIP decode must be as close to the exact answer as the reference is (x1.25) and
    # within 2x that floor of the reference itself.
    exact = V.VaeDecoderOracle(cfg, W, dtype=torch.float32).decode_to_pixel(g["latent"].float(), use_cache=True, chunk_size=1)
    floor = rel_l2(ref, exact)
    mine = rel_l2(got, exact)
    print(f"bf16 noise floor (reference vs exact) {floor:.3e}; HIP vs exact {mine:.3e}")
    assert mine <= 1.25 * floor, (mine, floor)
    assert r <= 2.0 * floor and float(d.max()) < 0.1, (r, floor)


def test_decode_flows_are_bit_identical(tiny):
    """all-at-once, per-block streaming (chunk 1), chunk 2 and three frames per decoder call: same pixels, bit for bit."""
    g, cfg, W, vae = tiny
    lat = g["latent"].cuda()
    a = vae.decode_to_pixel(lat, use_cache=False)
    b = vae.decode_to_pixel(lat, use_cache=True, chunk_size=1)
    c = vae.decode_to_pixel(lat, use_cache=True, chunk_size=2)
    assert torch.equal(a, b) and torch.equal(a, c)
    again = vae.decode_to_pixel(lat, use_cache=False)
    assert torch.equal(a, again), "decode is not deterministic"


def test_decoder_layers_teacher_forced(tiny):
    """Each decoder stage on the oracle's own inputs (errors do not accumulate through the net): residual block, attention
    block, temporal + spatial upsampler, residual block with the 1x1x1 shortcut.  Two calls per stage from a clean cache:
    the first chunk (zero history / 'Rep') and a two-frame chunk on the live feature cache."""
    g, cfg, W, vae = tiny
    orc = V.VaeDecoderOracle(cfg, W)
    dec = vae.model
    cl = lambda t: t[0].permute(1, 2, 3, 0).contiguous()                  # [1,c,t,h,w] -> [t,h,w,c]
    gen = torch.Generator().manual_seed(11)

    def check(kind, p, cin, cout, h, w):
        orc.clear_cache()
        dec.clear_cache()
        for t in (1, 2):
            x = rnd(gen, 1, cin, t, h, w)
            xc = cl(x).cuda()
            if kind == "res":
                ref, got = orc._res(p, x, cin, cout), dec._res(p, xc.clone(), cin, cout)
            elif kind == "attn":
                ref, got = orc._attn(p, x), dec._attn(p, xc)
            else:
                ref, got = orc._upsample(kind, p, x), dec._upsample(kind, p, xc)
            # attention: scores and probabilities pass through bf16 between the three launches (flash kernels keep them
            # in fp32), which flips more last bits of the block output — still inside the 2-ulp element bound
            assert_bf16_parity(got.cpu(), cl(ref), max_ulp=2, max_mismatch_frac=0.4 if kind == "attn" else 0.2, rel=3e-3,
                               floor=1.0, what=f"{kind} {p} chunk of {t}")

    check("res", "decoder.middle.0", 128, 128, 8, 12)
    check("attn", "decoder.middle.1", 128, 128, 8, 12)
    check("up3d", "decoder.upsamples.3", 128, 64, 8, 12)
    check("res", "decoder.upsamples.4", 64, 128, 16, 24)          # 1x1x1 shortcut
    check("up2d", "decoder.upsamples.11", 64, 32, 10, 14)
    dec.clear_cache()


def test_pipeline_takes_the_hip_vae(tiny, tmp_path):
    """The pipelines' `vae=` seam with the real decoder: T2V decodes the whole clip (1 + 4 (T - 1) frames), per-block
    streaming hands 9 uint8 frames per 3-frame block (each `decode_to_pixel(use_cache=True)` call restarts the stream, as
    upstream, wrapper.py:147-165) and the frames equal the CPU oracle's decode of the same latents within the noise floor."""
    import yaml
    import wan_oracle as O
    from inferix_amd.core import DecodeMode
    from inferix_amd.pipeline import SelfForcingPipeline
    g, vcfg, VW, vae = tiny
    cfg = O.tiny_config()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                independent_first_frame=False, context_noise=0, timestep_shift=5.0, kv_cache_tokens=21 * cfg.frame_seqlen,
                latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim,
                                  ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim,
                                  num_heads=cfg.num_heads, num_layers=cfg.num_layers, eps=cfg.eps))
    path = tmp_path / "sf.yaml"
    path.write_text(yaml.safe_dump(conf))
    pe = torch.randn(1, cfg.text_len, cfg.text_dim, generator=torch.Generator().manual_seed(5)).to(BF).cuda()
    pipe = SelfForcingPipeline(str(path), text_encoder=lambda text_prompts: {"prompt_embeds": pe.expand(len(text_prompts), -1, -1)},
                               vae=vae)
    W = O.init_weights(cfg, seed=0)
    ck = tmp_path / "ckpt.pt"
    torch.save({"generator": {"model." + k: v for k, v in W.items()}}, ck)
    pipe.load_checkpoint(str(ck), use_ema=False)
    pipe.setup_devices(low_memory=False, verbose=False)

    torch.manual_seed(3)
    video = pipe.run_text_to_video(["a prompt"], num_output_frames=6, num_samples=1)
    assert video.shape == (1, 21, 3, 8 * cfg.latent_h, 8 * cfg.latent_w) and 0.0 <= float(video.min()) <= float(video.max()) <= 1.0
    torch.manual_seed(3)
    _, lat = pipe._run_inference(["a prompt"], 6, 1, decode_mode=DecodeMode.NO_DECODE, return_latents=True)
    orc = V.VaeDecoderOracle(vcfg, VW)
    ref = (orc.decode_to_pixel(lat.cpu(), use_cache=True, chunk_size=2) * 0.5 + 0.5).clamp(0, 1)
    assert rel_l2(video.float().cpu(), ref) < 2e-2

    got = []
    torch.manual_seed(3)
    streamed = pipe.run_streaming_generation(["p0"], stream_callback=got.append, num_segments=1, segment_length=6, num_samples=1)
    H, Wd = 8 * cfg.latent_h, 8 * cfg.latent_w
    assert len(got) == 2 and all(f.dtype == torch.uint8 and tuple(f.shape) == (9, H, Wd, 3) for f in got)
    assert streamed.shape == (1, 18, H, Wd, 3)
    blk = (orc.decode_to_pixel(lat[:, :3].cpu(), use_cache=True, chunk_size=1) * 0.5 + 0.5).clamp(0, 1).permute(0, 1, 3, 4, 2)
    assert rel_l2(streamed[:, :9].float(), blk) < 2e-2


@pytest.mark.parametrize("h,w", [(60, 104), (90, 160)])
def test_full_size_against_oracle_on_device(h, w):
    """Full geometry (dim 96; latent 60 x 104 -> 480 x 832 and 90 x 160 -> 720 x 1280): two latent frames (first-chunk rule + live cache) through the
    HIP decoder against the SAME oracle code executed by torch on the GPU (MIOpen / rocBLAS kernels: an independent
    implementation of every conv), both compared with the fp32 evaluation as the exact answer."""
    from inferix_amd.vae import HipWanVAEWrapper, synthetic_decoder_state_dict
    cfg = V.VaeConfig()
    W = synthetic_decoder_state_dict(seed=3)
    lat = torch.randn(1, 2, 16, h, w, generator=torch.Generator().manual_seed(9)).to(BF)
    vae = HipWanVAEWrapper(W)
    got = vae.decode_to_pixel(lat.cuda(), use_cache=True, chunk_size=1)
    assert got.shape == (1, 5, 3, 8 * h, 8 * w) and torch.isfinite(got).all()
    again = vae.decode_to_pixel(lat.cuda(), use_cache=False)
    assert torch.equal(got, again)

    def on_device(dtype):
        orc = V.VaeDecoderOracle(cfg, {k: v.cuda() for k, v in W.items()}, dtype=dtype)
        orc.mean, orc.std = orc.mean.cuda(), orc.std.cuda()
        return orc.decode_to_pixel(lat.cuda().to(dtype), use_cache=True, chunk_size=1).float()

    ref = on_device(BF)
    exact = on_device(torch.float32)
    floor, mine, r = rel_l2(ref, exact), rel_l2(got, exact), rel_l2(got, ref)
    print(f"{8 * h}p: bf16 noise floor (torch bf16 vs fp32) {floor:.3e}; HIP vs fp32 {mine:.3e}; HIP vs torch bf16 {r:.3e}")
    assert mine <= 1.25 * floor + 1e-3 and r <= 2.0 * floor + 1e-3
    del vae
    torch.cuda.empty_cache()


# ---- encoder (image-to-video start frames) ------------------------------------------------------------------------
def test_encoder_matches_reference_golden():
    from inferix_amd.vae import HipWanVAEWrapper
    g = golden("vae_encode.npz")
    cfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    EW = V.make_encoder_params(cfg, int(g["seed"]))
    assert weights_checksum(EW) == int(g["weights_checksum"])
    DW = V.make_decoder_params(cfg, 4242)
    vae = HipWanVAEWrapper({**DW, **EW}, dim=cfg.dim)
    exact_orc = V.VaeEncoderOracle(cfg, EW, dtype=torch.float32)
    for name, x, ref in (("5 frames", g["video"], g["latent"]), ("1 frame", g["video"][:, :, :1], g["latent_first_frame"])):
        got = vae.encode_to_latent(x.cuda()).cpu()
        assert got.shape == ref.shape and got.dtype == torch.float32
        exact = exact_orc.encode_to_latent(x.float())
        floor, mine, r = rel_l2(ref, exact), rel_l2(got, exact), rel_l2(got, ref)
        print(f"encode [{name}]: bf16 noise floor {floor:.3e}; HIP vs fp32 {mine:.3e}; HIP vs reference {r:.3e}")
        assert mine <= 1.25 * floor + 1e-3 and r <= 2.0 * floor + 1e-3
        assert torch.equal(got, vae.encode_to_latent(x.cuda()).cpu()), "encode is not deterministic"
    # round trip through the HIP decoder keeps the geometry of the pipelines: [B, T', 16, h, w] -> [B, 1 + 4 (T' - 1), 3, 8h, 8w]
    lat = vae.encode_to_latent(g["video"].cuda())
    vid = vae.decode_to_pixel(lat.to(BF).cuda(), use_cache=True, chunk_size=1)
    assert vid.shape == (1, 5, 3, 64, 96)


def test_encoder_downsamplers_teacher_forced():
    """The two places where the encoder does not run a kernel in its native geometry: the stride-2 spatial conv (full
    resolution + odd-position sampling) and the stride-2 temporal conv (one launch per output frame)."""
    from inferix_amd.vae import HipWanVAEEncoder
    g = golden("vae_encode.npz")
    cfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    EW = V.make_encoder_params(cfg, int(g["seed"]))
    enc = HipWanVAEEncoder(EW, dim=cfg.dim)
    orc = V.VaeEncoderOracle(cfg, EW)
    gen = torch.Generator().manual_seed(2)
    cl = lambda t: t[0].permute(1, 2, 3, 0).contiguous()
    for kind, p, c, h, w in (("down2d", "encoder.downsamples.2", 32, 18, 26), ("down3d", "encoder.downsamples.5", 64, 16, 24),
                             ("down3d", "encoder.downsamples.5", 64, 9, 13)):
        orc.clear_cache()
        enc.clear_cache()
        for t in (1, 4, 4):
            x = rnd(gen, 1, c, t, h, w)
            ref = orc._downsample(kind, p, x)
            got = enc._downsample(kind, p, cl(x).cuda())
            assert_bf16_parity(got.cpu(), cl(ref), max_ulp=1, floor=1.0, what=f"{kind} {h}x{w} chunk of {t}")


def test_all_hip_image_to_video(tmp_path):
    """Image-to-video through the plugin class with nothing but HIP components on the data path: the start image goes through
    `HipWanVAEWrapper.encode_to_latent`, becomes the first latent frame (prefilled at t = 0, `independent_first_frame`), three
    more frames are denoised behind it and the clip is decoded: 4 latent frames -> 13 video frames."""
    import yaml
    import wan_oracle as O
    from inferix_amd.core import DecodeMode
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.vae import HipWanVAEWrapper
    vcfg = V.VaeConfig(dim=32)
    VW = {**V.make_decoder_params(vcfg, 4242), **V.make_encoder_params(vcfg, 4343)}
    vae = HipWanVAEWrapper(VW, dim=vcfg.dim)
    cfg = O.tiny_config()
    conf = dict(denoising_step_list=[1000, 500], warp_denoising_step=True, num_frame_per_block=3, independent_first_frame=True,
                context_noise=0, timestep_shift=5.0, kv_cache_tokens=22 * cfg.frame_seqlen,
                latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim,
                                  ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim,
                                  num_heads=cfg.num_heads, num_layers=cfg.num_layers, eps=cfg.eps))
    path = tmp_path / "sf_i2v.yaml"
    path.write_text(yaml.safe_dump(conf))
    pe = torch.randn(1, cfg.text_len, cfg.text_dim, generator=torch.Generator().manual_seed(5)).to(BF).cuda()
    pipe = SelfForcingPipeline(str(path), text_encoder=lambda text_prompts: {"prompt_embeds": pe.expand(len(text_prompts), -1, -1)},
                               vae=vae)
    W = O.init_weights(cfg, seed=0)
    ck = tmp_path / "ckpt.pt"
    torch.save({"generator": {"model." + k: v for k, v in W.items()}}, ck)
    pipe.load_checkpoint(str(ck), use_ema=False)
    pipe.setup_devices(low_memory=False, verbose=False)
    image = (torch.rand(1, 3, 1, 8 * cfg.latent_h, 8 * cfg.latent_w, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(BF)
    torch.manual_seed(4)
    video = pipe.run_image_to_video(["a prompt"], None, num_output_frames=4, image=image.cuda())
    assert video.shape == (1, 13, 3, 8 * cfg.latent_h, 8 * cfg.latent_w) and torch.isfinite(video).all()
    # the first latent frame of the clip IS the encoded image: decoding it alone reproduces the clip's first video frame
    lat0 = vae.encode_to_latent(image.cuda()).to(BF)
    first = (vae.decode_to_pixel(lat0.cuda(), use_cache=True, chunk_size=1) * 0.5 + 0.5).clamp(0, 1)
    assert torch.equal(video[:, :1].float().cpu(), first.float().cpu())
    ref0 = V.VaeEncoderOracle(vcfg, VW).encode_to_latent(image)
    assert rel_l2(lat0.float().cpu(), ref0) < 2e-2


def test_conv3d_ping_pong_equals_lock_step_on_random_shapes(ops):
    """The persistent ping-pong kernel walks cursors over tiles, stages and kernel rows, masks halo columns by tile position and splits
    its requests between wave groups; the lock-step kernel of round 1 derives everything per tile.  Same K order, same epilogue rounding:
    on 40 random launches — frames from 1 x 3 to 70 x 200 pixels (one tile that is both first and last column, ragged last rows /
    columns, several tiles per workgroup), 32 .. 288 input and 96 / 192 / 288 output channels, 1 .. 6 output frames, temporal kernel
    1 / 3 with zero frames in front, fused upsampling, with and without residual, planar and channels-last inputs, shuffled frame
    slots — the two must agree BIT FOR BIT."""
    g = torch.Generator().manual_seed(2024)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    for case in range(40):
        ups = ri(0, 3) == 0
        kt = 1 if ups else (3 if ri(0, 3) else 1)
        cin, cout = 32 * ri(1, 9), 96 * ri(1, 3)
        h, w = (ri(1, 35), ri(2, 100)) if ups else (ri(1, 70), ri(3, 200))
        t = ri(1, 6)
        res = (not ups) and ri(0, 1) == 1
        planar = (not ups) and ri(0, 1) == 1
        n_in = t + kt - 1
        ho, wo = (2 * h, 2 * w) if ups else (h, w)
        frames = rnd(g, n_in + 1, h, w, cin).cuda()
        slots = torch.randperm(n_in + 1, generator=g)[:n_in].tolist()
        if kt == 3 and ri(0, 1):
            slots[0] = -1
            if ri(0, 1):
                slots[1] = -1
        wt = rnd(g, kt * 9, cin // 32, cout, 32, scale=(cin * kt * 9) ** -0.5).cuda()
        b = rnd(g, cout, scale=0.1).cuda() if ri(0, 3) else None
        residual = rnd(g, t, ho, wo, cout).cuda() if res else None
        xin = ops.to_planar(frames) if planar else frames
        outs = []
        for variant in (0, 1):
            y = torch.full((t + 1, ho, wo, cout), 7.0, dtype=BF, device="cuda")
            out_slots = list(range(1, t + 1))
            ops.set_option("conv_variant", variant)
            try:
                ops.conv3d_cl(xin, slots, wt, b, kt=kt, ks=3, y=y, out_slots=out_slots, upsample=ups, residual=residual)
            finally:
                ops.set_option("conv_variant", 0)
            outs.append(y)
        what = f"case {case}: kt{kt} ups{int(ups)} {cin}->{cout} @{h}x{w} t{t} res{int(res)} planar{int(planar)} slots{slots}"
        assert torch.isfinite(outs[0].float()).all(), what
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), what
        assert float((outs[0][0].float() - 7.0).abs().max()) == 0.0, what + ": a slot that was not named was written"

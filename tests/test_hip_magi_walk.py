"""GPU: `ChunkSchedule.walk` (per-chunk generator on `forward_velocities` + one `ifx_magi_integrate` per step) against `ChunkSchedule.run`,
its hand-outs against tests/golden/magi_walk.npz (the reference's own `integrate_velocity`), its freedom from host synchronisation,
`generate_per_chunk` through the tiny `HipVideoDiTModel` against the bf16 oracle model, and `MagiPipeline` end to end."""
import functools
from types import SimpleNamespace

import pytest
import torch

from fixture_io import golden

pytestmark = pytest.mark.gpu
C_LAT, H_LAT, W_LAT, CAP_L, CAP_C = 4, 4, 6, 5, 8


def _stub_model(cfg_number=1, threshold=0.3, in_channels=C_LAT):
    """A deterministic model in torch on the device: the velocity is a fixed function of the input, the timestep of every range, the
    caption rows (through their mask) and the caption-dropout flag.  Only `forward` is its own: the dispatcher, the three guidance
    forwards and `forward_velocities` are `HipVideoDiTModel`'s, so the two loops drive the very code the real model runs."""
    from inferix_amd.magi.model import HipVideoDiTModel

    class Stub:
        forward_dispatcher = HipVideoDiTModel.forward_dispatcher
        _dispatch_3cfg = HipVideoDiTModel._dispatch_3cfg
        forward_3cfg = HipVideoDiTModel.forward_3cfg
        generate_kv_range_for_uncondition = HipVideoDiTModel.generate_kv_range_for_uncondition
        _forward_velocities = HipVideoDiTModel.forward_velocities

        def __init__(self):
            self.device = torch.device("cuda", torch.cuda.current_device())
            self.model_config = SimpleNamespace(patch_size=2, t_patch_size=1, in_channels=in_channels, caption_max_length=CAP_L)
            self.engine_config = SimpleNamespace(shortcut_mode="", distill_nearly_clean_chunk_threshold=threshold)
            self.runtime_config = SimpleNamespace(cfg_number=cfg_number, noise2clean_kvrange=[4, 3, 2, 2], clean_chunk_kvrange=1, clean_t=0.9999,
                                                  cfg_t_range=[0.0, 0.3], prev_chunk_scales=[1.5, 1.0], text_scales=[7.5, 0.0])
            self.patch_size, self.t_patch_size = 2, 1
            g = torch.Generator().manual_seed(9)
            self.w = {"y_embedder.null_caption_embedding": torch.randn(CAP_L, CAP_C, generator=g).to(self.device)}
            self.forwards, self.nearly, self.bins = 0, [], []

        def forward(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None, inference_params=None, **kw):
            self.forwards += 1
            N, _, T, _, _ = x.shape
            dn = t.shape[1]
            assert y.shape[0] == N * dn and xattn_mask.shape[0] == N * dn and T % dn == 0 and kw["denoising_range_num"] == dn
            per = T // dn
            cap = (y.float().reshape(N * dn, -1, y.shape[-1]) * xattn_mask.float().reshape(N * dn, -1, 1)).sum((1, 2)).reshape(N, dn)
            cap = torch.tanh(0.05 * cap).repeat_interleave(per, dim=1).reshape(N, 1, T, 1, 1)
            tt = t.float().repeat_interleave(per, dim=1).reshape(N, 1, T, 1, 1)
            drop = caption_dropout_mask.float().reshape(-1, 1, 1, 1, 1)
            return 0.5 * torch.sin(1.3 * x.float() + 2.0 * tt) + 0.25 * cap + 0.125 * drop - 0.1 * tt

        def forward_velocities(self, **kw):
            self.nearly.append(bool(kw["nearly_clean"]))
            self.bins.append(kw["cfg_bins"])
            return self._forward_velocities(**kw)

    return Stub()


def _inputs(chunk_num, cw, prefix_frames, seed, channels=C_LAT):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(1, channels, chunk_num * cw, H_LAT, W_LAT, generator=g)
    y = torch.randn(2, chunk_num, CAP_L, CAP_C, generator=g)
    masks = torch.zeros(2, chunk_num, CAP_L)
    masks[0, :, :4] = 1
    masks[1, :, :2] = 1
    prefix = None
    if prefix_frames:
        p0 = torch.randn(1, channels, prefix_frames, H_LAT, W_LAT, generator=g)
        prefix = torch.cat([p0, p0], 0).cuda()
    return torch.cat([x0, x0], 0).cuda(), y.cuda(), masks.cuda(), prefix


def _frame_range(view, clip):
    hw = clip.shape[3] * clip.shape[4]
    assert view.shape[0] == 1 and view.shape[1] == clip.shape[1] and view.stride() == clip[0:1].stride()
    start = (view.storage_offset() - clip.storage_offset()) // hw
    return start, start + view.shape[2]


def _walk_vs_run(case, cfg_number):
    from inferix_amd.magi.schedule import ChunkSchedule
    fx = golden("magi_walk.npz")
    num_steps, window, chunk_num, cw, prefix_frames = [int(v) for v in fx[f"c{case}_args"]]
    sch = ChunkSchedule(num_steps, window, chunk_num, cw, chunk_offset=prefix_frames // cw)
    x, y, masks, prefix = _inputs(chunk_num, cw, prefix_frames, seed=70 + case)
    ip = SimpleNamespace(update_kv_cache=False)
    want = sch.run(_stub_model(cfg_number), x.clone(), y, masks, ip, prefix_video=prefix)
    model = _stub_model(cfg_number)
    clip = x.clone()
    got = [(idx, _frame_range(v, clip), v.clone()) for idx, v in sch.walk(model, clip, y, masks, ip, prefix_video=prefix)]
    assert torch.equal(clip, want), "walk and run leave different clips"
    assert torch.equal(clip[0], clip[1])
    handed = [r[1:] for r in fx[f"c{case}_hand_out"].tolist() if r[0]]
    assert [[idx, a, b] for idx, (a, b), _ in got] == handed, ([(i, r) for i, r, _ in got], handed)
    for idx, (a, b), chunk in got:
        assert torch.equal(chunk, clip[0:1, :, a:b]), f"chunk {idx} was written after it was handed out"
    return model


def test_walk_equals_run_cfg1_with_and_without_the_nearly_clean_forward():
    model = _walk_vs_run(0, 1)
    assert True in model.nearly and False in model.nearly, model.nearly
    assert len(model.nearly) == 12 and all(b is None for b in model.bins)


def test_walk_equals_run_cfg3_both_guidance_bins():
    model = _walk_vs_run(0, 3)
    hit = {b for bins in model.bins for b in bins}
    assert hit == {0, 1}, model.bins
    assert model.forwards == 3 * 12


@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_walk_equals_run_short_clips_windows_and_prefixes(case):
    """Fewer chunks than the window, a window of one, and the three prefixes: one frame (image to video), a chunk plus a frame, whole
    chunks only."""
    _walk_vs_run(case, 1)


def _count_syncs(monkeypatch, counted):
    """Wrap what makes the host wait for the device, for a build on which the sync debug mode does nothing: the reads (`item`, `cpu`,
    `tolist`, `numpy`, the scalar conversions, `.to` across devices without `non_blocking`), the operators whose output size is read off
    the device (`nonzero`, `masked_select`, `unique`) and the blocking uploads (`torch.tensor` / `torch.as_tensor` with a GPU device)."""
    def method(name):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, **k):
            if self.is_cuda:
                counted.append(name)
            return orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__", "nonzero", "masked_select", "unique"):
        method(name)
    to = torch.Tensor.to

    def to_wrapped(self, *a, **k):
        out = to(self, *a, **k)
        if out.is_cuda != self.is_cuda and not (k.get("non_blocking", False) and self.is_pinned()):
            counted.append("to")
        return out
    monkeypatch.setattr(torch.Tensor, "to", to_wrapped)

    def function(name):
        orig = getattr(torch, name)

        def wrapped(*a, **k):
            out = orig(*a, **k)
            if name in ("tensor", "as_tensor"):
                if out.is_cuda and not (a and isinstance(a[0], torch.Tensor) and a[0].is_cuda):
                    counted.append("torch." + name)
            elif any(isinstance(v, torch.Tensor) and v.is_cuda for v in a):
                counted.append("torch." + name)
            return out
        monkeypatch.setattr(torch, name, wrapped)
    for name in ("tensor", "as_tensor", "nonzero", "masked_select", "unique"):
        function(name)


def test_sync_counter_sees_the_synchronising_calls(monkeypatch):
    """The fallback of the test below, exercised whether or not it is needed: each kind of wait is counted, what does not wait is not."""
    counted = []
    _count_syncs(monkeypatch, counted)
    d = torch.arange(4, device="cuda")
    quiet = [d + 1, d[1:3].clone(), torch.zeros(2, device="cuda"), torch.ones(3).pin_memory().to("cuda", non_blocking=True), d.to(torch.float32)]
    assert not counted and len(quiet) == 5, counted
    d.sum().item(), d.cpu(), d.to("cpu"), d.nonzero(), torch.masked_select(d, d > 1), torch.tensor([1, 2], device="cuda")
    torch.ones(2).to("cuda"), bool(d[0] == 0), d.tolist()
    assert counted[:7] == ["item", "cpu", "to", "nonzero", "torch.masked_select", "torch.tensor", "to"], counted
    assert "__bool__" in counted and "tolist" in counted


@pytest.mark.parametrize("cfg_number", [1, 3])
def test_walk_does_not_wait_for_the_device(monkeypatch, cfg_number):
    """The stub-model walk with every synchronising call made an error, from behind the clip's one host copy (`host_grid`) to the last
    hand-out, in both guidance modes: the nearly-clean re-forward (`cfg_number == 1`) and the three guidance forwards (`cfg_number == 3`)
    go through `HipVideoDiTModel`'s own `forward_velocities`, `forward_3cfg` and `generate_kv_range_for_uncondition`.  A `.item()` or a
    blocking upload put back into a step fails this test."""
    from inferix_amd.magi import schedule as S
    before = torch.cuda.get_sync_debug_mode()
    probe = torch.ones(3, device="cuda").sum()
    effective = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            effective = True
        if effective:                                      # a blocking upload from pageable memory is a wait too
            with pytest.raises(RuntimeError):
                torch.tensor([1.0, 2.0], device="cuda")
    finally:
        torch.cuda.set_sync_debug_mode(before)
    counted = []
    if not effective:                                      # the mode does nothing on this build: count the synchronising calls instead
        _count_syncs(monkeypatch, counted)
    print("sync check by", "torch.cuda.set_sync_debug_mode('error')" if effective else "counting wrapped synchronising calls")
    grid = S.host_grid
    copies = []

    def host_grid(*a):
        out = grid(*a)
        copies.append(1)
        counted.clear()
        if effective:
            torch.cuda.set_sync_debug_mode("error")        # from here on a wait for the device raises
        return out
    monkeypatch.setattr(S, "host_grid", host_grid)
    sch = S.ChunkSchedule(8, 4, 3, 2)
    x, y, masks, _ = _inputs(3, 2, 0, seed=90)
    model = _stub_model(cfg_number)
    chunks = []
    try:
        for idx, v in sch.walk(model, x, y, masks, SimpleNamespace(update_kv_cache=False)):
            chunks.append((idx, v.clone()))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert copies == [1] and not counted, counted
    assert [i for i, _ in chunks] == [0, 1, 2]
    if cfg_number == 1:
        assert True in model.nearly and False in model.nearly, model.nearly
    else:
        assert {b for bins in model.bins for b in bins} == {0, 1} and model.forwards == 36
    assert all(torch.isfinite(c).all() for _, c in chunks)


def test_walk_reproduces_the_reference_clip_from_its_recorded_velocities(monkeypatch):
    """tests/golden/magi_walk.npz holds, per case, the noise, the prefix, the velocity the reference's `integrate_velocity` was handed in
    every step and the clip it left (its own `integrate` and `try_pad_prefix_video`).  The same velocities through `walk` — the
    in-place prefix paste and `ifx_magi_integrate` — must leave that clip bit for bit, on the reference's time grid (`init_t` evaluated on
    the CPU as the fixture's generator evaluates it: `linspace` and the sd3 transform need not round alike on the device)."""
    from inferix_amd.magi import schedule as S
    fx = golden("magi_walk.npz")
    Cn, Hn, Wn = [int(v) for v in fx["geom"]]
    init_t = S.init_t
    monkeypatch.setattr(S, "init_t", lambda cfg, n, device="cpu", shortcut="": init_t(cfg, n, "cpu", shortcut).to(device))
    for c in range(int(fx["n_cases"])):
        num_steps, window, chunk_num, cw, prefix_frames = [int(v) for v in fx[f"c{c}_args"]]
        sch = S.ChunkSchedule(num_steps, window, chunk_num, cw, chunk_offset=prefix_frames // cw)
        vel = fx[f"c{c}_velocity"].cuda()

        class Recorded:
            model_config = SimpleNamespace(patch_size=1)
            engine_config = SimpleNamespace(shortcut_mode="")
            runtime_config = SimpleNamespace(cfg_number=1, noise2clean_kvrange=[], clean_chunk_kvrange=1, clean_t=0.9999)
            at = 0

            def forward_dispatcher(self, **kw):                # the prefix extraction pass: nothing to integrate
                assert kw["extract_prefix_video_feature"]

            def forward_velocities(self, **kw):
                n = kw["denoising_range_num"] - int(kw["fwd_extra_1st_chunk"])
                size = Cn * n * cw * Hn * Wn
                v = vel[self.at:self.at + size].reshape(1, Cn, n * cw, Hn, Wn)
                self.at += size
                return [(v, 0, 0, n - 1, [1.0] * n)]
        noise = fx[f"c{c}_noise"].cuda()
        clip = torch.cat([noise, noise], 0)
        prefix = fx[f"c{c}_prefix"].cuda().repeat(2, 1, 1, 1, 1) if prefix_frames else None
        model = Recorded()
        y, masks = torch.zeros(2, chunk_num, 2, 3, device="cuda"), torch.ones(2, chunk_num, 2, device="cuda")
        got = [(idx, _frame_range(v, clip)) for idx, v in sch.walk(model, clip, y, masks, None, prefix_video=prefix)]
        assert model.at == vel.numel(), (c, model.at, vel.numel())
        want = fx[f"c{c}_final"].cuda()
        assert torch.equal(clip[0:1], want) and torch.equal(clip[1:2], want), f"case {c}: walk leaves another clip than the reference"
        assert [[i, a, b] for i, (a, b) in got] == [r[1:] for r in fx[f"c{c}_hand_out"].tolist() if r[0]]


# ---- the tiny HIP model -------------------------------------------------------------------------------------------------------------
def _tiny():
    import magi_block_oracle as MB
    import magi_model_oracle as MM
    from test_hip_magi_model import _config
    cfg = MM.tiny_model_config()
    EW = MM.init_embedder_weights(cfg, 5)
    Ws = [MB.init_layer_weights(cfg.layer, 40 + li) for li in range(cfg.num_layers)]
    config = _config(cfg)
    config.engine_config.shortcut_mode = "8,16,16"
    config.engine_config.distill_nearly_clean_chunk_threshold = 0.3
    return cfg, EW, Ws, config


def _runtime(num_frames):
    return SimpleNamespace(cfg_number=1, noise2clean_kvrange=[4, 3, 2, 2], clean_chunk_kvrange=1, clean_t=0.9999, num_steps=8, window_size=4,
                           chunk_width=2, num_frames=num_frames, temporal_downsample_factor=4, video_size_h=64, video_size_w=96)


@functools.lru_cache(maxsize=None)
def _tiny_request(with_prefix: bool):
    """The request of test_chunk_schedule_rollout_vs_oracle_model — its configuration, weight seeds and noise (3 chunks x 2 frames of
    8 x 12, 8 steps in a window of 4) — with the caption rows `extract_feature_for_inference` packs, and the bf16 oracle model's clip for
    it (`_OracleModel` through `ChunkSchedule.run`, on the CPU, once)."""
    from inferix_amd.magi.prompt import extract_feature_for_inference
    from inferix_amd.magi.schedule import ChunkSchedule
    from test_hip_magi_model import _OracleModel
    cfg, EW, Ws, config = _tiny()
    chunk_num, cw, Hl, Wl = 3, 2, 8, 12
    tokens = cw * (Hl // 2) * (Wl // 2)
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(1, cfg.in_channels, chunk_num * cw, Hl, Wl, generator=g)
    caption = torch.randn(1, 1, cfg.caption_max_length, cfg.caption_channels, generator=g)
    cap_mask = torch.zeros(1, cfg.caption_max_length)
    cap_mask[:, :7] = 1
    prefix = torch.randn(1, cfg.in_channels, cw + 1, Hl, Wl, generator=g) if with_prefix else None
    # 3 chunks in all: 6 new latent frames, or 3 behind the 3 prefix frames
    config.runtime_config = _runtime(12 if with_prefix else 24)
    host = SimpleNamespace(model_config=config.model_config, runtime_config=config.runtime_config,
                           w={"y_embedder.null_caption_embedding": EW["y_embedder.null_caption_embedding"]})
    inp = extract_feature_for_inference(host, prefix, caption, cap_mask)
    assert tuple(inp.latent_size) == tuple(x0.shape) and inp.chunk_num == chunk_num
    om = _OracleModel(cfg, EW, Ws, config, chunk_num * tokens)
    sch = ChunkSchedule(8, 4, chunk_num, cw, chunk_offset=1 if with_prefix else 0)
    want = sch.run(om, torch.cat([x0, x0], 0), inp.y, inp.emb_masks, SimpleNamespace(update_kv_cache=False),
                   prefix_video=None if prefix is None else torch.cat([prefix, prefix], 0))
    return cfg, EW, Ws, config, x0, caption, cap_mask, prefix, want


@pytest.mark.parametrize("with_prefix", [False, True])
def test_generate_per_chunk_through_the_tiny_hip_model_vs_oracle_model(with_prefix):
    """`generate_per_chunk(..., noise=x)` through `HipVideoDiTModel`: three chunks (behind the chunk-plus-a-frame prefix: the frame the
    prefix leaves of chunk 1, then chunk 2), whose concatenation minus the noise is held to the bound of
    test_chunk_schedule_rollout_vs_oracle_model against the same bf16 oracle model: rel_l2 < 1e-2."""
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.schedule import generate_per_chunk
    from util import rel_l2
    cfg, EW, Ws, config, x0, caption, cap_mask, prefix, want = _tiny_request(with_prefix)
    sd = dict(EW)
    for li, W in enumerate(Ws):
        sd.update({f"videodit_blocks.layers.{li}.{k}": v for k, v in W.items()})
    model = HipVideoDiTModel(config, "cuda")
    model.load_state_dict(sd)
    chunks = [c.clone() for c in generate_per_chunk(model, None if prefix is None else prefix.cuda(), caption.cuda(), cap_mask.cuda(),
                                                    noise=x0.cuda())]
    frames = [c.shape[2] for c in chunks]
    first = 3 if with_prefix else 0
    assert frames == ([1, 2] if with_prefix else [2, 2, 2]), frames
    got = torch.cat(chunks, dim=2).cpu()
    assert got.shape == (1, cfg.in_channels, 6 - first, 8, 12) and torch.isfinite(got).all()
    r = rel_l2(got - x0[:, :, first:], want[0:1, :, first:] - x0[:, :, first:])
    print(f"generate_per_chunk through the tiny HIP model{' behind a prefix' if with_prefix else ''}: {len(chunks)} chunks, "
          f"HIP vs oracle on x_final - x_noise: {r:.3e}")
    assert r < 1e-2, r


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
class _Embedder:
    model_max_length = CAP_L

    def get_text_embeddings(self, prompts):
        g = torch.Generator().manual_seed(len(prompts[0]))
        m = torch.zeros(1, CAP_L)
        m[:, :3] = 1
        return torch.randn(1, CAP_L, CAP_C, generator=g).cuda(), m.cuda()


@functools.lru_cache(maxsize=None)
def _tiny_vae():
    """The smallest decoder of the ViT-VAE fixtures (two blocks of width 256, the weight seed of tests/golden/magi_vit_a / _b) beside the
    tiny encoder, which encodes the image's prefix latents: the VAE tests/test_hip_magi_vit_encoder.py builds."""
    import magi_vit_encoder_util as E
    import magi_vit_util as U
    from inferix_amd.magi.vae import HipMagiVAEDecoder
    cfg, wseed = E.TINY, U.CASES["magi_vit_b"][1]
    sd = {"decoder." + k: v for k, v in U.make_weights(cfg, wseed).items()}
    sd |= {"encoder." + k: v for k, v in E.make_encoder_weights(cfg, E.TILE_WEIGHT_SEED).items()}
    vae = HipMagiVAEDecoder(cfg.ctor_kwargs(), device="cuda:0")
    vae.load_state_dict(sd)
    return vae, cfg


@pytest.mark.parametrize("image", [False, True])
def test_magi_pipeline_frames_equal_the_per_chunk_decode(image):
    import magi_vit_encoder_util as E
    from inferix_amd.magi.prompt import get_txt_embeddings
    from inferix_amd.magi.schedule import generate_per_chunk
    from inferix_amd.magi.vae import VaeHelper, encode_prefix_video
    from inferix_amd.pipeline.magi import MagiPipeline
    vae, vcfg = _tiny_vae()
    dit = _stub_model(1, in_channels=vcfg.z_chans)
    rc = dit.runtime_config
    rc.num_steps, rc.window_size, rc.chunk_width, rc.num_frames, rc.temporal_downsample_factor = 8, 4, 2, 16, 4
    rc.video_size_h, rc.video_size_w, rc.fps, rc.scale_factor = 8 * H_LAT, 8 * W_LAT, 16, 0.5
    config = SimpleNamespace(model_config=dit.model_config, engine_config=dit.engine_config, runtime_config=rc)
    written = []
    pipe = MagiPipeline(config, dit=dit, vae=vae, embedder=_Embedder(), writer=lambda f, p, fps: written.append((f, p, fps)))
    pixels = E.make_pixels(63, (1, 8 * H_LAT, 8 * W_LAT, 3)).cuda() if image else None
    torch.manual_seed(5)
    frames = pipe.run_image_to_video("a prompt", image=pixels) if image else pipe.run_text_to_video("a prompt")
    n_chunks = 3 if image else 2
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (n_chunks * 8, 3, 8 * H_LAT, 8 * W_LAT) and frames.is_cuda
    assert len(written) == 1 and written[0][0] is frames and written[0][1:] == ("./output.mp4", 16)
    # the same request by hand, from the same noise
    cap, cap_mask = get_txt_embeddings("a prompt", config, _Embedder())
    prefix = encode_prefix_video(pixels, rc.fps, vae, rc.scale_factor) if image else None
    torch.manual_seed(5)
    chunks = [c.clone() for c in generate_per_chunk(dit, prefix, cap, cap_mask)]
    assert len(chunks) == n_chunks and all(tuple(c.shape) == (1, vcfg.z_chans, 2, H_LAT, W_LAT) for c in chunks)
    want = torch.cat([VaeHelper.decode(c / rc.scale_factor, vae, 256, 256, 0.25, 0, rc.fps // 2, True) for c in chunks], dim=0)
    assert torch.equal(frames, want)
    assert frames.float().std() > 1.0, "the decoded clip is flat"

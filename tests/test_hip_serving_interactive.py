"""InteractiveSessionBatch on the GPU, tiny synthetic model and VAE (the configuration of tests/test_hip_serving.py): given frames, a
prompt change, a join in the middle of a neighbour's block, an independent_first_frame config, and the frames each session streams.

The expected side is always `CausalInferencePipeline.inference(noise=, renoise=, text_prompts=, initial_latent=, NO_DECODE)` with the
noise and eps tensors drawn from `torch.Generator(device).manual_seed(seed)` in the documented order: per generated block one
`[1, n, C, H, W]` bf16 noise tensor, then S - 1 eps tensors of that shape.  Tolerance: the rule of tests/test_hip_serving.py — the
yardstick is the largest rel-L2 distance between a num_samples = 2 run of `inference` and its two solo runs; `torch.equal` when it is 0,
else distance <= 2 x yardstick.

Measured on an MI355X (profiles/r28_interactive_sessions.md): yardstick 0, every session of every scenario bit-identical."""
import pytest
import torch

import vae_oracle as V
import wan_oracle as O
from fixture_io import golden, weights_checksum
from util import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NFB, S = 3, 4


def make_pipe(tmp, independent_first_frame):
    import yaml
    from inferix_amd.pipeline import SelfForcingPipeline
    from inferix_amd.vae import HipWanVAEWrapper
    g = golden("vae_decode.npz")
    vcfg = V.VaeConfig(dim=int(g["cfg_dim"]))
    VW = V.make_decoder_params(vcfg, int(g["seed"]))
    assert weights_checksum(VW) == int(g["weights_checksum"])
    vae = HipWanVAEWrapper(VW, dim=vcfg.dim)
    cfg = O.tiny_config()
    conf = dict(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=NFB,
                independent_first_frame=independent_first_frame, context_noise=0, timestep_shift=5.0,
                kv_cache_tokens=21 * cfg.frame_seqlen, latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim,
                                  ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim,
                                  num_heads=cfg.num_heads, num_layers=cfg.num_layers, eps=cfg.eps))
    path = tmp / "sf.yaml"
    path.write_text(yaml.safe_dump(conf))
    gen = torch.Generator().manual_seed(5)
    embeds = {}

    def encoder(text_prompts):
        for p in text_prompts:
            if p not in embeds:
                e = torch.zeros(cfg.text_len, cfg.text_dim)
                n = 4 + len(embeds) * 5
                e[:n] = torch.randn(n, cfg.text_dim, generator=gen)
                embeds[p] = e.to(BF).cuda()
        return {"prompt_embeds": torch.stack([embeds[p] for p in text_prompts])}
    p = SelfForcingPipeline(str(path), text_encoder=encoder, vae=vae)
    ck = tmp / "ckpt.pt"
    torch.save({"generator": {"model." + k: v for k, v in O.init_weights(cfg, seed=0).items()}}, ck)
    p.load_checkpoint(str(ck), use_ema=False)
    p.setup_devices(low_memory=False, verbose=False)
    p.frame_hw = (8 * cfg.latent_h, 8 * cfg.latent_w)
    p.block_tokens = NFB * cfg.frame_seqlen
    return p


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    return make_pipe(tmp_path_factory.mktemp("isessions"), False)


@pytest.fixture(scope="module")
def pipe_iff(tmp_path_factory):
    return make_pipe(tmp_path_factory.mktemp("isessions_iff"), True)


def draws(p, seed, sizes):
    """What a session with `seed` draws for generated blocks of `sizes` frames: `(noise [1, sum, C, H, W], renoise list)`."""
    g = torch.Generator(device=p.device).manual_seed(seed)
    noise, eps = [], []
    for n in sizes:
        shape = [1, n, *p.latent_shape]
        noise.append(torch.randn(shape, generator=g, device=p.device, dtype=BF))
        eps += [torch.randn(shape, generator=g, device=p.device, dtype=BF).flatten(0, 1) for _ in range(S - 1)]
    return torch.cat(noise, dim=1), eps


def infer(p, prompts, noise, eps, initial_latent=None):
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    kvm = KVCacheManager(device=p.device)
    reqs = [KVCacheRequest(f"want{i}") for i in range(len(prompts))]
    out = p.pipeline.inference(noise=noise, text_prompts=prompts, kv_cache_manager=kvm, kv_cache_requests=reqs,
                               initial_latent=initial_latent, decode_mode=DecodeMode.NO_DECODE, renoise=eps)
    for r in reqs:
        if r.request_id in kvm.request_to_kv_caches:
            kvm.free(r)
    return out


def solo(p, prompt, seed, sizes, initial_latent=None):
    noise, eps = draws(p, seed, sizes)
    out = infer(p, [prompt], noise, eps, initial_latent)
    return out if initial_latent is None else out[:, initial_latent.shape[1]:]


@pytest.fixture(scope="module")
def yardstick(pipe):
    """The parent's own batching: num_samples = 2 against two num_samples = 1 runs of `inference` with the same noise and `renoise`
    tensors — the largest relative L2 distance between a batch row and its solo run."""
    T = 12
    g = torch.Generator().manual_seed(9)
    noise = torch.randn(2, T, *pipe.latent_shape, generator=g).to(BF).cuda()
    eps = [torch.randn(2, NFB, *pipe.latent_shape, generator=g).to(BF).cuda() for _ in range((S - 1) * T // NFB)]
    prompts = ["prompt A", "prompt B"]
    both = infer(pipe, prompts, noise, [e.flatten(0, 1) for e in eps])
    alone = [infer(pipe, [p], noise[i:i + 1], [e[i:i + 1].flatten(0, 1) for e in eps]) for i, p in enumerate(prompts)]
    torch.cuda.synchronize()
    return max(rel_l2(both[i:i + 1].cpu(), alone[i].cpu()) for i in range(2))


def check(name, got, want, yardstick):
    assert got.shape == want.shape and torch.isfinite(got.float()).all(), (name, got.shape, want.shape)
    d = rel_l2(got.cpu(), want.cpu())
    print(f"ISESSIONS|{name}: session vs inference {d:.3e}; yardstick (num_samples 2 vs 1) {yardstick:.3e}")
    if yardstick == 0.0:
        assert torch.equal(got, want), (name, d)
    else:
        assert d <= 2 * yardstick, (name, d, yardstick)


def streamed(p, session, cbs, latents, sizes, nv12):
    """The session's kept video and its callback blocks against the one-shot decode of `latents` `[1, T, C, h, w]`."""
    from inferix_amd import hip_ops as ops
    H, W = p.frame_hw
    u8 = p.pipeline.vae.model.fork().cached_decode_u8(latents.permute(0, 2, 1, 3, 4))
    assert tuple(u8.shape) == (1 + 4 * (latents.shape[1] - 1), H, W, 3)
    want = (ops.rgb8_to_yuv420(u8, layout="nv12") if nv12 else u8).cpu()
    video = session.stream.video()
    assert video.dtype == torch.uint8 and not video.is_cuda and video.shape[0] == 1
    assert torch.equal(video[0], want)
    assert [f.shape[0] for f in cbs] == [4 * sizes[0] - 3] + [4 * n for n in sizes[1:]]       # one callback per push, in order
    assert torch.equal(torch.cat(cbs, dim=0), want)


@pytest.fixture(scope="module")
def given_frames(pipe):
    """Scenario 1: A opened with 6 given latent frames (two prefill blocks) beside plain B, which is two blocks ahead; two steps."""
    from inferix_amd.serving import InteractiveSessionBatch
    model = pipe.pipeline.generator.model
    sb = InteractiveSessionBatch(pipe, max_sessions=2)
    given = (0.5 * torch.randn(1, 2 * NFB, *pipe.latent_shape, generator=torch.Generator().manual_seed(21))).to(BF)
    cbs = []
    b = sb.open("prompt B", seed=2)
    lat = {"a": [], "b": []}
    for _ in range(2):
        lat["b"].append(sb.step()[b].clone())
    a = sb.open("prompt A", seed=1, initial_latent=given, continuous=True, keep_video=True, stream_callback=lambda f: cbs.append(f.clone()))
    model.index_trace = []
    try:
        for _ in range(2):
            out = sb.step()
            assert list(out) == [b, a]
            lat["a"].append(out[a].clone())
            lat["b"].append(out[b].clone())
        trace = list(model.index_trace)
    finally:
        model.index_trace = None
    counts = (a.frames_done, a.block, a.forwards, b.forwards)
    sb.close_all()
    torch.cuda.synchronize()
    return dict(a=torch.cat(lat["a"], dim=1), b=torch.cat(lat["b"], dim=1), given=given.cuda(), trace=trace, counts=counts, session=a,
                cbs=cbs)


def test_given_frames(pipe, given_frames, yardstick):
    r = given_frames
    check("given frames, A", r["a"], solo(pipe, "prompt A", 1, [NFB] * 2, initial_latent=r["given"]), yardstick)
    check("given frames, B", r["b"], solo(pipe, "prompt B", 2, [NFB] * 4), yardstick)
    N = pipe.block_tokens
    # A's prefill at positions 0 and nfb beside B's first two denoising steps of its third block
    assert r["trace"][:4] == [(2 * N, 3 * N, 3 * N), (0, N, N), (2 * N, 3 * N, 3 * N), (N, 2 * N, 2 * N)]
    assert r["counts"] == (4 * NFB, 2, 2 + 2 * (S + 1), 4 * (S + 1))


def test_given_frames_stream(pipe, given_frames):
    r = given_frames
    streamed(pipe, r["session"], r["cbs"], torch.cat([r["given"], r["a"]], dim=1), [NFB] * 4, nv12=False)


@pytest.fixture(scope="module")
def prompt_change(pipe):
    """Scenario 2: A runs 2 blocks under "prompt A", then set_prompt(A, "prompt B"), 2 more steps; C beside it, undisturbed."""
    from inferix_amd.serving import InteractiveSessionBatch
    model = pipe.pipeline.generator.model
    sb = InteractiveSessionBatch(pipe, max_sessions=2)
    cbs = {"a": [], "c": []}
    a = sb.open("prompt A", seed=1, continuous=True, keep_video=True, pixel_format="nv12", stream_callback=lambda f: cbs["a"].append(f.clone()))
    c = sb.open("prompt C", seed=3, continuous=True, keep_video=True, stream_callback=lambda f: cbs["c"].append(f.clone()))
    lat = {"a": [], "c": []}

    def steps():
        for _ in range(2):
            out = sb.step()
            lat["a"].append(out[a].clone())
            lat["c"].append(out[c].clone())
    steps()
    sb.set_prompt(a, "prompt B")
    model.index_trace = []
    try:
        steps()
        trace = list(model.index_trace)
    finally:
        model.index_trace = None
    counts = (a.segment, a.block, a.frames_done, a.position, c.segment, c.position)
    sb.close_all()
    plain = InteractiveSessionBatch(pipe, max_sessions=1)
    s = plain.open("prompt A", seed=1)
    unchanged = plain.run(4)[s]
    plain.close_all()
    torch.cuda.synchronize()
    return dict(a=torch.cat(lat["a"], dim=1), c=torch.cat(lat["c"], dim=1), trace=trace, counts=counts, sessions=(a, c), cbs=cbs,
                unchanged=unchanged)


def test_prompt_change(pipe, prompt_change, yardstick):
    r = prompt_change
    first = solo(pipe, "prompt A", 1, [NFB] * 2)
    check("prompt change, A before", r["a"][:, :2 * NFB], first, yardstick)
    # the draws carry on: blocks 3 and 4 of the session's generator, under the new prompt, from A's own last nfb latents
    noise, eps = draws(pipe, 1, [NFB] * 4)
    want = infer(pipe, ["prompt B"], noise[:, 2 * NFB:], eps[2 * (S - 1):], initial_latent=r["a"][:, NFB:2 * NFB])[:, NFB:]
    check("prompt change, A after", r["a"][:, 2 * NFB:], want, yardstick)
    check("prompt change, C", r["c"], solo(pipe, "prompt C", 3, [NFB] * 4), yardstick)
    N = pipe.block_tokens
    assert r["trace"][:2] == [(0, N, N), (2 * N, 3 * N, 3 * N)]            # A's trace restarts at 0, C carries on
    assert r["counts"] == (1, 4, 4 * NFB, 3 * NFB, 0, 4 * NFB)
    assert torch.equal(r["a"][:, :2 * NFB], r["unchanged"][:, :2 * NFB])
    assert not torch.equal(r["a"][:, 2 * NFB:], r["unchanged"][:, 2 * NFB:])   # the prompt change shows


def test_prompt_change_stream(pipe, prompt_change):
    """The overlap is not pushed again and the decoder stream is not reset: the video is the one-shot decode of the unique latents."""
    r = prompt_change
    a, c = r["sessions"]
    streamed(pipe, a, r["cbs"]["a"], r["a"], [NFB] * 4, nv12=True)
    streamed(pipe, c, r["cbs"]["c"], r["c"], [NFB] * 4, nv12=False)


def test_join_in_the_middle_of_a_block(pipe, yardstick):
    """Scenario 3: A takes two forwards alone, B opens, both run until they have two blocks."""
    from inferix_amd.serving import InteractiveSessionBatch
    sb = InteractiveSessionBatch(pipe, max_sessions=2)
    a = sb.open("prompt A", seed=1)
    sb.advance(), sb.advance()
    b = sb.open("prompt B", seed=2)
    lat = {a: [], b: []}
    joined = None
    while min(a.block, b.block) < 2:
        done = sb.advance()
        if joined is None:
            joined = (a.forwards, b.forwards, a.phase, b.phase)
        for s, x in done.items():
            lat[s].append(x.clone())
    assert joined == (3, 1, ("DENOISE", 3), ("DENOISE", 1))            # B's first forward was A's third
    assert a.forwards - b.forwards == 2 and b.forwards == 2 * (S + 1)
    sb.close_all()
    check("mid-block join, A", torch.cat(lat[a][:2], dim=1), solo(pipe, "prompt A", 1, [NFB] * 2), yardstick)
    check("mid-block join, B", torch.cat(lat[b][:2], dim=1), solo(pipe, "prompt B", 2, [NFB] * 2), yardstick)


def test_two_sessions_prefill_together(pipe, yardstick):
    """Both rows of a forward in PREFILL: `[B, 1]` zeros as `inference` hands over, several frames per row."""
    from inferix_amd.serving import InteractiveSessionBatch
    sb = InteractiveSessionBatch(pipe, max_sessions=2)
    given = (0.5 * torch.randn(2, NFB, *pipe.latent_shape, generator=torch.Generator().manual_seed(22))).to(BF).cuda()
    a = sb.open("prompt A", seed=1, initial_latent=given[0:1])
    b = sb.open("prompt B", seed=2, initial_latent=given[1:2])
    out = sb.step()
    assert a.forwards == b.forwards == 1 + S + 1
    got = {s: out[s].clone() for s in (a, b)}
    sb.close_all()
    check("prefill together, A", got[a], solo(pipe, "prompt A", 1, [NFB], initial_latent=given[0:1]), yardstick)
    check("prefill together, B", got[b], solo(pipe, "prompt B", 2, [NFB], initial_latent=given[1:2]), yardstick)


def test_independent_first_frame(pipe_iff, yardstick):
    """Scenario 4: a fresh session (1-frame opening block) beside one opened with a 1-frame initial latent (blocks of nfb at once)."""
    from inferix_amd.serving import InteractiveSessionBatch, SessionBatch
    with pytest.raises(NotImplementedError, match="independent_first_frame"):
        SessionBatch(pipe_iff)
    p = pipe_iff
    sb = InteractiveSessionBatch(p, max_sessions=2)
    first = (0.5 * torch.randn(1, 1, *p.latent_shape, generator=torch.Generator().manual_seed(23))).to(BF).cuda()
    a = sb.open("prompt A", seed=1)
    b = sb.open("prompt B", seed=2, initial_latent=first)
    lat = {a: [], b: []}
    for _ in range(2):
        for s, x in sb.step().items():
            lat[s].append(x.clone())
    assert [x.shape[1] for x in lat[a]] == [1, NFB] and [x.shape[1] for x in lat[b]] == [NFB, NFB]
    assert (a.frames_done, b.frames_done) == (1 + NFB, 1 + 2 * NFB)
    sb.close_all()
    check("independent first frame, fresh", torch.cat(lat[a], dim=1), solo(p, "prompt A", 1, [1, NFB]), yardstick)
    check("independent first frame, given", torch.cat(lat[b], dim=1), solo(p, "prompt B", 2, [NFB, NFB], initial_latent=first), yardstick)

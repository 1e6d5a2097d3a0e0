"""SessionBatch on the host: a stub generator (row-local arithmetic, records every call) behind the real CausalInferencePipeline,
scheduler, KVCacheManager and per-layer cache adapters.  What is checked is the bookkeeping: who is in which forward at which position,
join and leave, the noise of a session not depending on its neighbours, the refusals, the caches of a closed session."""
from types import SimpleNamespace

import pytest
import torch

from inferix_amd.kvcache_manager.model import SelfForcingKVCacheManagerFactory
from inferix_amd.pipeline import CausalInferencePipeline
from inferix_amd.schedulers import FlowMatchScheduler
from inferix_amd.serving import SessionBatch

LAYERS, NF, FSL, LATENT = 2, 3, 6, [4, 4, 6]            # frame_seq_length 6 = (4 / 2) * (6 / 2)
STEPS = [1000, 750, 500]


class StubGenerator:
    """x0 = x / 2 per row: a session's result depends on its own rows only, so whatever differs between a joint and a solo run is the
    batch's doing.  Keeps what `HipWanDiffusionWrapper.forward` is called with."""

    def __init__(self):
        blocks = [SimpleNamespace(kv_cache_manager=SelfForcingKVCacheManagerFactory.create_manager(l, 2, 128, enable_kv_offload=False))
                  for l in range(LAYERS)]
        self.model = SimpleNamespace(num_layers=LAYERS, local_attn_size=-1, text_len=4, blocks=blocks)
        self.parallel_config = SimpleNamespace(world_size=1, rank=0)
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.calls = []

    def get_scheduler(self):
        return self.scheduler

    def __call__(self, noisy_image_or_video, conditional_dict, timestep, kv_cache_meta, crossattn_cache_meta, current_start,
                 kv_cache_manager, kv_cache_requests):
        ragged = isinstance(current_start, list)
        B = noisy_image_or_video.shape[0]
        assert len(kv_cache_requests) == B == len(conditional_dict["prompt_embeds"]) and tuple(timestep.shape) == (B, NF)
        if ragged:
            assert len(current_start) == len(kv_cache_meta) == len(crossattn_cache_meta) == B and B >= 2
            assert all(len(m) == LAYERS for m in kv_cache_meta + crossattn_cache_meta)
        else:
            assert B == 1 and len(kv_cache_meta) == LAYERS and isinstance(kv_cache_meta[0], dict)
        self.calls.append(SimpleNamespace(start=list(current_start) if ragged else current_start,
                                          requests=[r.request_id for r in kv_cache_requests], t=float(timestep.flatten()[0]),
                                          prompts=[float(e.flatten()[0]) for e in conditional_dict["prompt_embeds"]],
                                          x=noisy_image_or_video.clone(), kv_meta=kv_cache_meta, cross_meta=crossattn_cache_meta))
        return torch.zeros_like(noisy_image_or_video), noisy_image_or_video * 0.5


def make_pipe(**over):
    args = SimpleNamespace(denoising_step_list=list(STEPS), warp_denoising_step=False, num_frame_per_block=NF,
                           independent_first_frame=over.pop("independent_first_frame", False), context_noise=0, model_kwargs={},
                           frame_seq_length=FSL, kv_cache_tokens=12 * FSL)
    gen = StubGenerator()
    encoder = lambda text_prompts: {"prompt_embeds": torch.full((len(text_prompts), 4, 8), float(len(text_prompts[0])))}
    inner = CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=encoder, vae=None)
    pipe = SimpleNamespace(pipeline=inner, device=torch.device("cpu"), parallel_config=SimpleNamespace(world_size=over.pop("world_size", 1)),
                           latent_shape=LATENT, _pipeline_type=over.pop("pipeline_type", "causal"), config=args)
    assert not over
    return pipe, gen


def test_positions_join_and_leave():
    pipe, gen = make_pipe()
    sb = SessionBatch(pipe, max_sessions=4)
    a = sb.open("prompt A", seed=1)
    a_meta = (a.kv_meta, a.cross_meta)
    for _ in range(2):
        out = sb.step()
        assert list(out) == [a] and out[a].shape == (1, NF, *LATENT)
    b = sb.open("a longer prompt B", seed=2)             # joins at the next step, at ITS block 0
    b_meta = (b.kv_meta, b.cross_meta)
    for _ in range(3):
        out = sb.step()
        assert list(out) == [a, b]
    assert (a.block, b.block, a.frames_done, b.frames_done) == (5, 3, 15, 9)
    sb.close(a)
    out = sb.step()
    assert list(out) == [b] and b.block == 4 and a.closed and sb.sessions == [b]
    per_step = len(STEPS) + 1                            # the denoising steps and the clean-context re-run
    assert len(gen.calls) == 6 * per_step
    N = NF * FSL
    want = [0, N] + [[2 * N, 0], [3 * N, N], [4 * N, 2 * N]] + [3 * N]
    for i, c in enumerate(gen.calls):
        step, k = divmod(i, per_step)
        assert c.start == want[step], (i, c.start)
        assert c.requests == (["session_0"] if step < 2 else ["session_0", "session_1"] if step < 5 else ["session_1"])
        assert c.t == ([float(s) for s in STEPS] + [0.0])[k]          # one timestep for every row
        pa, pb = float(len("prompt A")), float(len("a longer prompt B"))
        assert c.prompts == ([pa] if step < 2 else [pa, pb] if step < 5 else [pb])
        if isinstance(c.start, list):                   # every session hands in ITS OWN meta lists
            assert c.kv_meta[0] is a_meta[0] and c.kv_meta[1] is b_meta[0] and c.cross_meta[0] is a_meta[1] and c.cross_meta[1] is b_meta[1]
        else:
            mine = a_meta if step < 2 else b_meta
            assert c.kv_meta is mine[0] and c.cross_meta is mine[1]


def test_a_sessions_noise_does_not_depend_on_its_neighbours():
    pipe, gen = make_pipe()
    sb = SessionBatch(pipe)
    a = sb.open("A", seed=11)
    sb.step()
    sb.step()
    b = sb.open("B", seed=12)
    joint = sb.run(3)
    assert set(joint) == {a, b} and joint[b].shape == (1, 3 * NF, *LATENT)
    pipe2, gen2 = make_pipe()
    solo_batch = SessionBatch(pipe2)
    b2 = solo_batch.open("B", seed=12)
    solo = solo_batch.run(3)
    assert torch.equal(joint[b], solo[b2])
    # the generator saw the same rows for B in both runs: its opening noise and every re-noised input
    rows_joint = [c.x[1:2] for c in gen.calls if c.requests == ["session_0", "session_1"]]
    rows_solo = [c.x for c in gen2.calls]
    assert len(rows_joint) == len(rows_solo) == 3 * (len(STEPS) + 1)
    assert all(torch.equal(x, y) for x, y in zip(rows_joint, rows_solo))
    # and another seed is another video
    pipe3, _ = make_pipe()
    other = SessionBatch(pipe3)
    b3 = other.open("B", seed=13)
    assert not torch.equal(other.run(3)[b3], solo[b2])


def test_close_frees_the_sessions_caches_only():
    pipe, gen = make_pipe()
    sb = SessionBatch(pipe)
    a, b = sb.open("A", seed=1), sb.open("B", seed=2)
    live = sb.kvm.request_to_kv_caches
    assert a.request.request_id in live and b.request.request_id in live
    sb.step()
    sb.close(a)
    assert a.request.request_id not in live and b.request.request_id in live
    assert a.kv_meta == [] and a.prompt_embeds is None and a.closed
    sb.close(a)                                          # closing twice is harmless
    assert sb.step().keys() == {b}
    sb.close_all()
    assert not live and sb.sessions == [] and sb.step() == {}
    c = sb.open("C", seed=3)                             # a batch that emptied takes new sessions
    assert c.index == 2 and c.request.request_id == "session_2" and sb.step().keys() == {c}


def test_refusals_name_their_reason():
    with pytest.raises(NotImplementedError, match="few-step pipeline"):
        SessionBatch(make_pipe(pipeline_type="causal_diffusion")[0])
    with pytest.raises(NotImplementedError, match="world_size 2"):
        SessionBatch(make_pipe(world_size=2)[0])
    with pytest.raises(NotImplementedError, match="independent_first_frame"):
        SessionBatch(make_pipe(independent_first_frame=True)[0])
    with pytest.raises(ValueError, match="max_sessions must be positive"):
        SessionBatch(make_pipe()[0], max_sessions=0)
    sb = SessionBatch(make_pipe()[0], max_sessions=2)
    with pytest.raises(NotImplementedError, match="initial_latent"):
        sb.open("p", initial_latent=torch.zeros(1, 3, *LATENT))
    with pytest.raises(ValueError, match="need continuous=True"):
        sb.open("p", stream_callback=lambda frames: None)
    with pytest.raises(ValueError, match="need continuous=True"):
        sb.open("p", pixel_format="nv12")
    with pytest.raises(RuntimeError, match="continuous=True needs a vae"):
        sb.open("p", continuous=True)
    assert sb.sessions == [] and not sb.kvm.request_to_kv_caches      # a refused open leaves nothing behind
    sb.open("p"), sb.open("q")
    with pytest.raises(RuntimeError, match="2 sessions are live and max_sessions is 2"):
        sb.open("r")

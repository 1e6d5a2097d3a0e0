"""InteractiveSessionBatch on the host: the stub generator of tests/test_serving_host.py (row-local arithmetic, records every call) behind
the real CausalInferencePipeline, scheduler, KVCacheManager and per-layer cache adapters.  What is checked is the bookkeeping of the
work items: who is in which forward, at which position, at which timestep, with which prompt; the draws of a session's generator; the
refusals."""
from types import SimpleNamespace

import pytest
import torch

from inferix_amd.kvcache_manager.model import SelfForcingKVCacheManagerFactory
from inferix_amd.pipeline import CausalInferencePipeline
from inferix_amd.schedulers import FlowMatchScheduler, const_tag
from inferix_amd.serving import InteractiveSessionBatch, SessionBatch

LAYERS, NF, FSL, LATENT = 2, 3, 6, [4, 4, 6]            # frame_seq_length 6 = (4 / 2) * (6 / 2)
STEPS = [1000, 750, 500]
S = len(STEPS)
N = NF * FSL


class StubGenerator:
    """x0 = x / 2 per row.  Keeps what `HipWanDiffusionWrapper.forward` is called with; the cache meta is moved as the model moves it,
    so that a reset shows."""

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
        B, n = noisy_image_or_video.shape[:2]
        assert len(kv_cache_requests) == B == len(conditional_dict["prompt_embeds"]) and tuple(timestep.shape) in ((B, n), (B, 1))
        if ragged:
            assert len(current_start) == len(kv_cache_meta) == len(crossattn_cache_meta) == B and B >= 2
        else:
            assert B == 1 and len(kv_cache_meta) == LAYERS and isinstance(kv_cache_meta[0], dict)
        metas = kv_cache_meta if ragged else [kv_cache_meta]
        cross = crossattn_cache_meta if ragged else [crossattn_cache_meta]
        starts = current_start if ragged else [current_start]
        self.calls.append(SimpleNamespace(start=list(current_start) if ragged else current_start,
                                          requests=[r.request_id for r in kv_cache_requests], t=timestep, tag=const_tag(timestep),
                                          t_rows=[float(r[0]) for r in timestep], t_shape=tuple(timestep.shape),
                                          prompts=[float(e.flatten()[0]) for e in conditional_dict["prompt_embeds"]],
                                          x=noisy_image_or_video.clone(), init=[c[0]["is_init"] for c in cross],
                                          ends=[int(m[0]["global_end_index"]) for m in metas]))
        for m, c, st in zip(metas, cross, starts):
            for layer in range(LAYERS):
                m[layer]["global_end_index"] = torch.tensor([st + n * FSL])
                m[layer]["local_end_index"] = torch.tensor([st + n * FSL])
                c[layer]["is_init"] = True
        return torch.zeros_like(noisy_image_or_video), noisy_image_or_video * 0.5


def make_pipe(independent_first_frame=False, vae=None):
    args = SimpleNamespace(denoising_step_list=list(STEPS), warp_denoising_step=False, num_frame_per_block=NF,
                           independent_first_frame=independent_first_frame, context_noise=0, model_kwargs={},
                           frame_seq_length=FSL, kv_cache_tokens=24 * FSL)
    gen = StubGenerator()
    encoder = lambda text_prompts: {"prompt_embeds": torch.full((len(text_prompts), 4, 8), float(len(text_prompts[0])))}
    inner = CausalInferencePipeline(args, "cpu", generator=gen, text_encoder=encoder, vae=vae)
    pipe = SimpleNamespace(pipeline=inner, device=torch.device("cpu"), parallel_config=SimpleNamespace(world_size=1),
                           latent_shape=LATENT, _pipeline_type="causal", config=args)
    return pipe, gen


def rows_of(gen, request):
    """(call index, row, call) of every forward the request took part in."""
    return [(k, c.requests.index(request), c) for k, c in enumerate(gen.calls) if request in c.requests]


def solo(prompt, seed, blocks, **kw):
    pipe, gen = make_pipe(**kw)
    sb = InteractiveSessionBatch(pipe)
    s = sb.open(prompt, seed=seed)
    return sb.run(blocks)[s], gen


def test_step_alone_makes_the_forwards_of_session_batch():
    """No given frames, no prompt change, no advance(): call for call what SessionBatch.step makes."""
    def scenario(cls):
        pipe, gen = make_pipe()
        sb = cls(pipe, max_sessions=4)
        a = sb.open("prompt A", seed=1)
        outs = [sb.step(), sb.step()]
        b = sb.open("a longer prompt B", seed=2)
        outs += [sb.step() for _ in range(3)]
        sb.close(a)
        outs.append(sb.step())
        return gen, [[(s.index, lat.clone()) for s, lat in o.items()] for o in outs], (a, b)
    old, old_out, _ = scenario(SessionBatch)
    new, new_out, (a, b) = scenario(InteractiveSessionBatch)
    assert len(old.calls) == len(new.calls) == 6 * (S + 1)
    for c, d in zip(old.calls, new.calls):
        assert c.requests == d.requests and c.start == d.start and c.prompts == d.prompts
        assert d.t_shape == c.t_shape and torch.equal(c.t, d.t) and c.t.dtype == d.t.dtype
        assert d.tag is not None and d.tag == c.tag                       # the tagged constant: the modulation and sigma memos hit
        assert torch.equal(c.x, d.x)
    for o, p in zip(old_out, new_out):
        assert [i for i, _ in o] == [i for i, _ in p] and all(torch.equal(x, y) for (_, x), (_, y) in zip(o, p))
    assert (a.block, b.block, a.frames_done, b.frames_done, a.forwards, b.forwards) == (5, 4, 15, 12, 5 * (S + 1), 4 * (S + 1))
    assert a.segment == b.segment == 0 and b.phase is None


def test_a_session_joins_at_the_next_forward():
    pipe, gen = make_pipe()
    sb = InteractiveSessionBatch(pipe)
    a = sb.open("A", seed=11)
    assert a.phase is None
    assert sb.advance() == {} and a.phase == ("DENOISE", 1)
    assert sb.advance() == {} and a.phase == ("DENOISE", 2)
    b = sb.open("prompt B", seed=12)
    assert sb.advance() == {} and (a.phase, b.phase) == (("RERUN", None), ("DENOISE", 1))
    third = gen.calls[2]
    assert third.requests == ["session_0", "session_1"] and third.start == [0, 0]
    assert third.t_shape == (2, NF) and third.t_rows == [float(STEPS[2]), float(STEPS[0])] and third.tag is None
    assert torch.equal(third.t, torch.tensor([[STEPS[2]] * NF, [STEPS[0]] * NF]))
    lat = {a: [], b: []}
    while min(a.block, b.block) < 2:
        for s, x in sb.advance().items():
            assert x.shape == (1, NF, *LATENT)
            lat[s].append(x.clone())
    assert (b.forwards, a.forwards - b.forwards) == (2 * (S + 1), 2) and b.block == 2
    # a finished its second block two forwards before b: it has moved on into its third
    assert a.block == 2 and a.phase == ("DENOISE", 2)
    for s, (prompt, seed) in ((a, ("A", 11)), (b, ("prompt B", 12))):
        want, gen_solo = solo(prompt, seed, 2)
        assert torch.equal(torch.cat(lat[s][:2], dim=1), want)
        mine = rows_of(gen, s.request.request_id)[:2 * (S + 1)]
        alone = gen_solo.calls
        assert len(mine) == len(alone) == 2 * (S + 1)
        for (_, row, c), d in zip(mine, alone):            # the same noise, the same re-noised inputs, the same timesteps
            assert torch.equal(c.x[row:row + 1], d.x) and c.t_rows[row] == d.t_rows[0]
            assert (c.start[row] if isinstance(c.start, list) else c.start) == d.start
    # b projected its text in the forward it joined in, a did not project again
    assert third.init == [True, False]


def test_given_frames_are_prefilled_at_t0_and_not_returned():
    pipe, gen = make_pipe()
    sb = InteractiveSessionBatch(pipe)
    b = sb.open("B", seed=2)
    sb.step()
    given = torch.randn(1, 2 * NF, *LATENT, generator=torch.Generator().manual_seed(3))
    a = sb.open("A", seed=1, initial_latent=given)
    assert a.phase == ("PREFILL", None) and a.frames_done == 0
    calls = len(gen.calls)
    out = sb.step()
    assert list(out) == [b, a] and out[a].shape == (1, NF, *LATENT)
    assert (a.frames_done, a.position, a.block, b.frames_done) == (3 * NF, 3 * NF, 1, 2 * NF)
    mine = rows_of(gen, "session_1")
    assert [k - calls for k, _, _ in mine] == list(range(2 + S + 1))
    for j, (_, row, c) in enumerate(mine[:2]):             # the two prefill forwards, beside b's first two denoising steps
        assert c.requests == ["session_0", "session_1"] and c.start == [N, j * N]
        assert c.t_rows == [float(STEPS[j]), 0.0] and c.t_shape == (2, NF)
        assert torch.equal(c.x[row:row + 1], given[:, j * NF:(j + 1) * NF].to(torch.bfloat16))
    assert [(c.start[row] if isinstance(c.start, list) else c.start) for _, row, c in mine[2:]] == [2 * N] * (S + 1)
    assert [c.t_rows[row] for _, row, c in mine[2:]] == [float(t) for t in STEPS] + [0.0]
    # b sat out the forwards after its block was done
    assert [c.requests for c in gen.calls[calls + S + 1:]] == [["session_1"]] * 2
    # a's generated block: the draws of a session without given frames (PREFILL draws nothing)
    first_block, _ = solo("A", 1, 1)
    assert torch.equal(out[a], first_block)
    # a lone session's prefill: [1, 1] zeros, the uniform call
    pipe2, gen2 = make_pipe()
    sb2 = InteractiveSessionBatch(pipe2)
    c = sb2.open("C", seed=4, initial_latent=given[:, :NF])
    sb2.advance()
    assert gen2.calls[0].t_shape == (1, 1) and gen2.calls[0].t_rows == [0.0] and gen2.calls[0].start == 0
    assert gen2.calls[0].t.dtype == torch.int64 and c.frames_done == NF and c.forwards == 1
    # two sessions in prefill together: [B, 1] zeros
    d = sb2.open("D", seed=5, initial_latent=given)
    e = sb2.open("E", seed=6, initial_latent=given[:, NF:])
    sb2.close(c)
    sb2.advance()
    assert gen2.calls[1].t_shape == (2, 1) and gen2.calls[1].t_rows == [0.0, 0.0] and gen2.calls[1].start == [0, 0]
    assert (d.phase, e.phase) == (("PREFILL", None), None)


def test_given_frames_shape_rules():
    sb = InteractiveSessionBatch(make_pipe()[0])
    with pytest.raises(ValueError, match="multiple of num_frame_per_block"):
        sb.open("p", initial_latent=torch.zeros(1, NF + 1, *LATENT))
    with pytest.raises(ValueError, match=r"initial_latent must be \[1, n, 4, 4, 6\]"):
        sb.open("p", initial_latent=torch.zeros(2, NF, *LATENT))
    with pytest.raises(ValueError, match="initial_latent or image, not both"):
        sb.open("p", initial_latent=torch.zeros(1, NF, *LATENT), image=torch.zeros(1, 3, 1, 32, 48))
    with pytest.raises(RuntimeError, match="needs a vae with an encoder"):
        sb.open("p", image=torch.zeros(1, 3, 1, 32, 48))
    iff = InteractiveSessionBatch(make_pipe(independent_first_frame=True)[0])
    with pytest.raises(ValueError, match=r"1 \+ k \* num_frame_per_block"):
        iff.open("p", initial_latent=torch.zeros(1, NF, *LATENT))
    assert sb.sessions == [] and iff.sessions == [] and not sb.kvm.request_to_kv_caches       # a refused open leaves nothing behind
    with pytest.raises(ValueError, match="keep_frames must be non-negative"):
        InteractiveSessionBatch(make_pipe()[0], keep_frames=-1)


def test_image_goes_through_the_vae_encoder():
    seen = []

    def encode_to_latent(image):
        seen.append(image)
        return torch.full((1, NF, *LATENT), 0.25)
    pipe, gen = make_pipe(vae=SimpleNamespace(encode_to_latent=encode_to_latent))
    sb = InteractiveSessionBatch(pipe)
    image = torch.zeros(1, 3, 1, 32, 48)
    a = sb.open("A", image=image)
    sb.advance()
    assert seen[0] is image and a.frames_done == NF
    assert torch.equal(gen.calls[0].x, torch.full((1, NF, *LATENT), 0.25, dtype=torch.bfloat16)) and gen.calls[0].t_rows == [0.0]


def test_independent_first_frame_config():
    with pytest.raises(NotImplementedError, match="independent_first_frame"):
        SessionBatch(make_pipe(independent_first_frame=True)[0])
    pipe, gen = make_pipe(independent_first_frame=True)
    sb = InteractiveSessionBatch(pipe)
    a = sb.open("A", seed=1)
    out = sb.step()
    assert out[a].shape == (1, 1, *LATENT) and (a.frames_done, a.block) == (1, 1)
    assert all(c.x.shape[1] == 1 and c.start == 0 for c in gen.calls) and len(gen.calls) == S + 1
    b = sb.open("B", seed=2)                               # its opening block has 1 frame, a's second one NF
    before = len(gen.calls)
    done = sb.advance()
    assert done == {} and len(gen.calls) == before + 2     # two forwards: one per frame count
    first, second = gen.calls[before:]
    assert (first.requests, first.x.shape[1], first.start) == (["session_0"], NF, FSL)
    assert (second.requests, second.x.shape[1], second.start) == (["session_1"], 1, 0)
    out = sb.step()
    assert out[a].shape == (1, NF, *LATENT) and out[b].shape == (1, 1, *LATENT)
    out = sb.step()                                        # from here on both make NF frames: one forward each time
    assert out[b].shape == (1, NF, *LATENT) and gen.calls[-1].requests == ["session_0", "session_1"]
    assert gen.calls[-1].start == [(1 + NF) * FSL, FSL]
    # given frames: the first one alone, then a block
    c = sb.open("C", seed=3, initial_latent=torch.zeros(1, 1 + NF, *LATENT))
    assert [it.n for it in c._queue] == [1, NF]
    solo_first, _ = solo("B", 2, 2, independent_first_frame=True)
    assert solo_first.shape == (1, 1 + NF, *LATENT)


def test_set_prompt_falls_due_at_the_block_boundary():
    pipe, gen = make_pipe()
    sb = InteractiveSessionBatch(pipe, keep_frames=2 * NF)
    a, c = sb.open("prompt A", seed=1), sb.open("C", seed=3)
    lat = [sb.step()[a].clone()]
    sb.advance()                                           # a block in flight ...
    sb.set_prompt(a, "never used", overlap_frames=0)
    sb.set_prompt(a, "a new prompt B", overlap_frames=NF)  # ... replaces the pending change, and falls due after the block
    assert a.prompt == "prompt A" and a.segment == 0
    lat.append(sb.step()[a].clone())
    assert a.segment == 0 and a.prompt == "prompt A" and (a.position, a.block) == (2 * NF, 2)
    assert all(c_.prompts[0] == float(len("prompt A")) for c_ in gen.calls)
    before = len(gen.calls)
    out = sb.step()
    assert (a.segment, a.prompt, a.block, a.frames_done, a.position) == (1, "a new prompt B", 3, 3 * NF, 2 * NF)
    assert (c.segment, c.block, c.position) == (0, 3, 3 * NF)
    new = gen.calls[before:]
    assert len(new) == 1 + S + 1
    pre = new[0]                                           # the prefill of a's last NF latents at position 0, t = 0, new prompt
    assert pre.requests == ["session_0", "session_1"] and pre.start == [0, 2 * N] and pre.t_rows == [0.0, float(STEPS[0])]
    assert pre.ends[0] == 0 and pre.init == [False, True]  # meta reset: the index state is back at 0, the text is projected again
    assert torch.equal(pre.x[0:1], lat[1]) and pre.prompts == [float(len("a new prompt B")), 1.0]
    for k, call in enumerate(new[1:S + 1]):
        assert call.start == [N, 2 * N] and call.t_rows == [float(STEPS[k]), float(STEPS[k + 1]) if k + 1 < S else 0.0]
        assert call.prompts[0] == float(len("a new prompt B")) and call.init == [True, True]
    assert new[-1].requests == ["session_0"] and new[-1].start == N and new[-1].t_rows == [0.0]
    assert out[a].shape == (1, NF, *LATENT)
    # the neighbour's rows are those of its solo run; a's draws carried on (no reseed): its noise is the solo run's third block's
    want_c, gen_c = solo("C", 3, 3)
    mine = rows_of(gen, "session_1")
    assert len(mine) == len(gen_c.calls) == 3 * (S + 1)
    assert all(torch.equal(x.x[row:row + 1], y.x) and x.t_rows[row] == y.t_rows[0] for (_, row, x), y in zip(mine, gen_c.calls))
    _, gen_a = solo("prompt A", 1, 3)
    assert torch.equal(new[1].x[0:1], gen_a.calls[2 * (S + 1)].x)
    # overlap_frames: within keep_frames, a multiple of the block; the default is keep_frames
    with pytest.raises(ValueError, match="exceeds keep_frames"):
        sb.set_prompt(a, "x", overlap_frames=3 * NF)
    with pytest.raises(ValueError, match="divisible by block_size"):
        sb.set_prompt(a, "x", overlap_frames=NF - 1)
    sb.set_prompt(a, "x")
    assert a._pending == ("x", 2 * NF)
    sb.close(a)
    with pytest.raises(RuntimeError, match="is closed"):
        sb.set_prompt(a, "y")


def test_set_prompt_uses_the_frames_that_exist():
    pipe, gen = make_pipe()
    sb = InteractiveSessionBatch(pipe, keep_frames=2 * NF)
    a = sb.open("A", seed=1)
    sb.set_prompt(a, "prompt B")                           # nothing made yet: a plain start under the new prompt
    sb.step()
    assert (a.segment, a.position, a.forwards) == (1, NF, S + 1) and gen.calls[0].prompts == [float(len("prompt B"))]
    sb.set_prompt(a, "prompt CC")                          # asks for 2 NF, NF exist
    sb.step()
    assert (a.segment, a.position, a.frames_done, a.forwards) == (2, 2 * NF, 2 * NF, 2 * (S + 1) + 1)
    iff_pipe, iff_gen = make_pipe(independent_first_frame=True)
    iff = InteractiveSessionBatch(iff_pipe)                # keep_frames NF: the valid overlaps are 0 and 1
    b = iff.open("B", seed=2)
    iff.step(), iff.step()
    with pytest.raises(ValueError, match=r"0 or 1 \+ k \* num_frame_per_block"):
        iff.set_prompt(b, "x", overlap_frames=2)
    iff.set_prompt(b, "x")
    assert b._pending == ("x", 1)
    before = len(iff_gen.calls)
    out = iff.step()
    assert iff_gen.calls[before].x.shape[1] == 1 and iff_gen.calls[before].start == 0 and out[b].shape == (1, NF, *LATENT)
    assert (b.position, b.frames_done) == (1 + NF, 1 + 2 * NF)


def test_close_in_the_middle_of_a_block():
    pipe, gen = make_pipe()
    sb = InteractiveSessionBatch(pipe)
    a, b = sb.open("A", seed=1), sb.open("B", seed=2)
    sb.advance(), sb.advance()
    assert a.phase == ("DENOISE", 2)
    sb.close(a)
    live = sb.kvm.request_to_kv_caches
    assert a.request.request_id not in live and b.request.request_id in live
    assert a.closed and a.phase is None and a._x is None and a.kv_meta == []
    out = sb.step()
    assert list(out) == [b] and b.block == 1 and b.forwards == S + 1
    want, _ = solo("B", 2, 1)
    assert torch.equal(out[b], want)
    assert [c.requests for c in gen.calls[2:]] == [["session_1"]] * 2

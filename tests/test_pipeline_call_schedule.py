"""The host-side call schedule of the three Wan inner pipelines, pinned call by call (no GPU; control flow only).

A recording stand-in generator logs every generator call, every per-layer cache call, every re-noise and every block callback of a
tiny clip; the logs are compared with the literals in tests/golden/pipeline_call_schedule.json.  Those were recorded by running this
file's own drivers with IFX_RECORD_CALL_SCHEDULE=1 at the commit BEFORE the pipelines were moved onto
`inferix_amd/pipeline/block_loop.py`, so they state what the three hand-written copies did.

A timestep is logged as (value, shape, dtype, tagged, object number): the object number counts distinct tensor OBJECTS in order of first
appearance, so a `_timestep` cache hit across blocks shows as a repeated number."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import pytest
import torch

from inferix_amd.core import DecodeMode
from inferix_amd.kvcache_manager import KVCacheRequest
from inferix_amd.pipeline import CausalDiffusionInferencePipeline, CausalInferencePipeline, CausVidInferencePipeline
from inferix_amd.schedulers import FlowMatchScheduler, const_tag

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_call_schedule.json")
RECORD = os.environ.get("IFX_RECORD_CALL_SCHEDULE", "") == "1"
STEPS = [1000, 750, 500, 250]
FSL = 24                                                     # frame_seq_length of the stand-in geometry


class _Log(list):
    """The call log, with the bookkeeping that turns tensors and managers into literals."""

    def __init__(self):
        super().__init__()
        self.tensors = []                                    # kept alive: an object number is never reused
        self.managers = {}

    def ts(self, t):
        for n, u in enumerate(self.tensors):
            if u is t:
                break
        else:
            n = len(self.tensors)
            self.tensors.append(t)
        return [round(float(t.flatten()[0]), 3), list(t.shape), str(t.dtype), const_tag(t) is not None, n]

    def kvm(self, m):
        return self.managers[id(m)]


class _Manager:
    """Stand-in KVCacheManager: a name, and `free` logged."""

    def __init__(self, log, name):
        self.log = log
        log.managers[id(self)] = name

    def free(self, req):
        self.log.append(["free", self.log.kvm(self), req.request_id])


class _Block:
    """Stand-in transformer block: its per-layer cache manager logs what it is asked for, with every keyword."""

    def __init__(self, log, layer):
        self.log, self.layer, self.kv_cache_manager, self._init = log, layer, self, False

    def _cache_call(self, what, kv_cache_manager, kv_cache_request, **kw):
        self.log.append([what, self.layer, self.log.kvm(kv_cache_manager), kv_cache_request.request_id,
                         sorted((k, str(v)) for k, v in kw.items())])

    def allocate_kv_cache(self, **kw):
        self._cache_call("allocate_kv_cache", **kw)

    def allocate_crossattn_cache(self, **kw):
        self._cache_call("allocate_crossattn_cache", **kw)

    def clear_cache(self, **kw):
        self._cache_call("clear_cache", **kw)

    @property
    def is_cross_attn_init(self):
        return self._init

    @is_cross_attn_init.setter
    def is_cross_attn_init(self, v):                         # the CausVid pipeline resets the flag on the block
        self.log.append(["is_cross_attn_init", self.layer, v])
        self._init = v


class _Gen(torch.nn.Module):
    """Recording generator.  `style`: "wan" returns (flow, x0), "causvid" x0 alone.  The model has THREE blocks and num_layers = 2, so
    a pipeline that walks `num_transformer_blocks` and one that walks `model.blocks` log different cache calls."""

    def __init__(self, log, style="wan", passthrough_add_noise=True):
        super().__init__()
        self.log, self.style, self.inside = log, style, "call"
        self.model = SimpleNamespace(num_layers=2, local_attn_size=-1, text_len=16, num_frame_per_block=1,
                                     blocks=[_Block(log, i) for i in range(3)])
        self.parallel_config = None
        self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        real = self.scheduler.add_noise

        def add_noise(x0, eps, t):
            log.append(["add_noise", list(x0.shape)] + log.ts(t))
            return real(x0, eps, t) if passthrough_add_noise else x0
        self.scheduler.add_noise = add_noise

    def get_scheduler(self):
        return self.scheduler

    def forward(self, noisy_image_or_video, conditional_dict, timestep, current_start, kv_cache_manager, kv_cache_requests,
                kv_cache_meta=None, crossattn_cache_meta=None, **slots):
        x = noisy_image_or_video
        meta = None if kv_cache_meta is None else [[int(m["global_end_index"]), int(m["local_end_index"]), str(m["global_end_index"].device)]
                                                   for m in kv_cache_meta]
        cross = None if crossattn_cache_meta is None else [m["is_init"] for m in crossattn_cache_meta]
        self.log.append([self.inside, current_start, list(x.shape)] + self.log.ts(timestep)
                        + [list(conditional_dict["prompt_embeds"]), self.log.kvm(kv_cache_manager), [r.request_id for r in kv_cache_requests],
                           meta, cross, sorted(slots.items())])
        return x * 0.5 if self.style == "causvid" else (x, x * 0.5)


class _PairGen(_Gen):
    def forward_pair(self, first, second):
        self.inside = "pair.first"
        a = self.forward(**first)
        self.inside = "pair.second"
        b = self.forward(**second)
        self.inside = "call"
        return a, b


class _CfgGen(_Gen):
    def forward_cfg(self, cond_kw, uncond_kw):
        self.inside = "cfg.cond"
        a = self.forward(**cond_kw)[0]
        self.inside = "cfg.uncond"
        b = self.forward(**uncond_kw)[0]
        self.inside = "call"
        return a, b


def _encoder(text_prompts):
    return {"prompt_embeds": tuple(text_prompts)}


def _latents(b, frames, seed):
    return torch.randn(b, frames, 4, 2, 2, generator=torch.Generator().manual_seed(seed))


def _args(**kw):
    return SimpleNamespace(denoising_step_list=list(STEPS), warp_denoising_step=True, num_frame_per_block=3,
                           independent_first_frame=False, context_noise=0, frame_seq_length=FSL, kv_cache_tokens=504, **kw)


# ---------------------------------------------------------------------------------------------- the three drivers
def run_causal(prefill: bool, pair: bool):
    log = _Log()
    gen = (_PairGen if pair else _Gen)(log)
    pipe = CausalInferencePipeline(_args(), "cpu", generator=gen, text_encoder=_encoder, vae=None)
    log.append(["denoising_step_list", [round(float(v), 3) for v in pipe.denoising_step_list], str(pipe.denoising_step_list.dtype)])
    out = pipe.inference(noise=_latents(1, 6, 0), text_prompts=["p"], kv_cache_manager=_Manager(log, "kvm"),
                         kv_cache_requests=[KVCacheRequest("r")], initial_latent=_latents(1, 3, 1) if prefill else None,
                         decode_mode=DecodeMode.NO_DECODE,
                         block_callback=lambda lat, i: log.append(["block_callback", i, list(lat.shape)]))
    log.append(["returned", list(out.shape), pipe.kv_cache_meta, pipe.crossattn_cache_meta])
    return pipe, log


def run_causvid():
    log = _Log()
    gen = _PairGen(log, style="causvid", passthrough_add_noise=False)   # a (B,) sigma does not broadcast over B * 3 rows: log it, skip it
    pipe = CausVidInferencePipeline(_args(), device="cpu", generator=gen, text_encoder=_encoder, vae=None)
    log.append(["denoising_step_list", [round(float(v), 3) for v in pipe.denoising_step_list], str(pipe.denoising_step_list.dtype)])
    outs = pipe.rollover(["first", "second"], [_latents(2, 6, 0), _latents(2, 6, 1)], _Manager(log, "kvm"), overlap_frames=3)
    log.append(["returned", [list(o.shape) for o in outs], pipe.is_kv_cache_initialized])
    return pipe, log


class _StubSolver:
    """`FlowUniPCSchedule` for the control flow: four host timesteps, `step_cfg` hands its latents back (the real one launches a kernel)."""

    def __init__(self, log):
        self.log, self.timesteps = log, torch.tensor([999, 750, 500, 250])

    def step_cfg(self, flow_cond, flow_uncond, guidance, t, latents, return_dict=False):
        self.log.append(["step_cfg", guidance, t])
        return (latents,)


def run_diffusion(prefill: bool, start_frame_index: int, cfg: bool = True):
    log = _Log()
    gen = (_CfgGen if cfg else _Gen)(log)
    pipe = CausalDiffusionInferencePipeline(_args(negative_prompt="neg", guidance_scale=3.0), "cpu", generator=gen,
                                            text_encoder=_encoder, vae=None)
    pipe._initialize_sample_scheduler = lambda noise: log.append(["fresh_solver"]) or _StubSolver(log)
    pos, neg = _Manager(log, "pos"), _Manager(log, "neg")
    out = pipe.inference(noise=_latents(1, 6, 0), text_prompts=["p"], kv_cache_manager_pos=pos, kv_cache_manager_neg=neg,
                         kv_cache_requests=[KVCacheRequest("r")], initial_latent=_latents(1, 3, 1) if prefill else None,
                         start_frame_index=start_frame_index, decode_mode=DecodeMode.NO_DECODE,
                         block_callback=lambda lat, i: log.append(["block_callback", i, list(lat.shape)]))
    log.append(["returned", list(out.shape), pipe.kv_cache_meta_pos is not None, pipe.crossattn_cache_meta_neg is not None])
    pipe.clear_cache(pos, neg, [KVCacheRequest("r")])
    log.append(["cleared", pipe.kv_cache_meta_pos, pipe.kv_cache_meta_neg, pipe.crossattn_cache_meta_pos, pipe.crossattn_cache_meta_neg])
    return pipe, log


CASES = {
    "causal": lambda: run_causal(False, False),
    "causal-pair": lambda: run_causal(False, True),
    "causal-prefill": lambda: run_causal(True, False),
    "causal-prefill-pair": lambda: run_causal(True, True),
    "causvid-rollover": run_causvid,
    "diffusion": lambda: run_diffusion(False, 0),
    "diffusion-prefill": lambda: run_diffusion(True, 0),
    "diffusion-start5": lambda: run_diffusion(False, 5),
    "diffusion-prefill-start5": lambda: run_diffusion(True, 5),
    "diffusion-prefill-unpaired": lambda: run_diffusion(True, 0, cfg=False),
}


def _check(case, got):
    """Compare a log with the recorded one, entry by entry (or, recording, write it: one entry per line)."""
    rec = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            rec = json.load(f)
    if RECORD:
        rec[case] = got
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(" " + json.dumps(e) for e in rec[k]) + "\n]"
                                        for k in sorted(rec)) + "\n}\n")
        return
    want = rec[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: entry {i}: got {g}, recorded {w}"
    assert len(got) == len(want), (len(got), len(want))


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_log_is_the_recorded_one(case):
    pipe, log = CASES[case]()
    got = json.loads(json.dumps(list(log)))                  # tuples -> lists, as the recorded file holds them
    _check(case, got)
    # the cache hits the log shows: every block walks the same (value, shape) and gets the same tensor OBJECT
    tagged = [tuple(map(str, e[3:8])) for e in got if e[0] in ("call", "pair.first", "pair.second", "cfg.cond", "cfg.uncond") and e[6]]
    by_key = {}
    for value, shape, dtype, _, number in tagged:
        assert by_key.setdefault((value, shape, dtype), number) == number
    assert len(by_key) < len(tagged)


@pytest.mark.parametrize("case,dtype,cap", [("causal", torch.int64, 32), ("causvid-rollover", torch.int64, 32),
                                            ("diffusion", torch.float32, 128)])
def test_timestep_cache_identity_default_dtype_and_eviction(case, dtype, cap):
    pipe, _ = CASES[case]()
    pipe._ts_cache.clear()
    a = pipe._timestep(500, (1, 3), "cpu")
    assert a.dtype == dtype and const_tag(a) == 500.0 and torch.equal(a, torch.full((1, 3), 500, dtype=dtype))
    assert pipe._timestep(500.0, [1, 3], "cpu") is a                         # the key is (float(value), tuple(shape), device, dtype)
    assert pipe._timestep(500, (1, 3), "cpu", dtype) is a
    assert pipe._timestep(500, (3,), "cpu") is not a and pipe._timestep(500, (1, 3), "cpu", torch.float64) is not a
    pipe._ts_cache.clear()
    for v in range(cap):
        pipe._timestep(v, (1,), "cpu")
    first = pipe._timestep(0, (1,), "cpu")
    assert len(pipe._ts_cache) == cap and pipe._timestep(0, (1,), "cpu") is first
    pipe._timestep(cap, (1,), "cpu")                                         # full: cleared, then the new entry alone
    assert len(pipe._ts_cache) == 1 and pipe._timestep(0, (1,), "cpu") is not first


@pytest.mark.parametrize("case,method", [("causal-pair", "forward_pair"), ("causvid-rollover", "forward_pair"),
                                         ("diffusion", "forward_cfg")])
def test_pairing_reads_args_then_the_environment_at_call_time(case, method, monkeypatch):
    pipe, _ = CASES[case]()
    monkeypatch.delenv("IFX_PAIR_FORWARDS", raising=False)
    assert hasattr(pipe.generator, method) and pipe._pairing() is True       # unset = on
    for env, want in (("0", False), ("off", False), ("false", False), ("1", True), ("", True)):
        monkeypatch.setenv("IFX_PAIR_FORWARDS", env)
        assert pipe._pairing() is want
    monkeypatch.setenv("IFX_PAIR_FORWARDS", "0")
    pipe.args.pair_forwards = True                                           # flipped on the live pipeline, as the benchmark does
    assert pipe._pairing() is True
    monkeypatch.setenv("IFX_PAIR_FORWARDS", "1")
    pipe.args.pair_forwards = False
    assert pipe._pairing() is False
    pipe.args.pair_forwards = None
    pipe.generator = _Gen(_Log())                                            # a generator without the paired entry point
    assert pipe._pairing() is False


# ---------------------------------------------------------------------------------------------- the wrapper's keyword mapping
class _RecModel:
    """Stand-in HipCausalWanModel: logs the keywords each entry point hands over."""

    def __init__(self):
        self.calls = []

    def _flow(self, kw):
        self.calls.append(sorted((k, v if isinstance(v, (int, str, type(None))) else type(v).__name__) for k, v in kw.items()))
        return kw["x"]

    def __call__(self, x, **kw):
        return self._flow(dict(kw, x=x))

    def forward_pair(self, first, second):
        return self._flow(first), self._flow(second)

    def forward_cfg(self, first, second):
        if second["kv_cache_manager"] is first["kv_cache_manager"]:
            raise ValueError("same manager")
        return self._flow(first), self._flow(second)


def _wrapper_kw(**over):
    kw = dict(noisy_image_or_video=torch.zeros(1, 3, 4, 2, 2), conditional_dict={"prompt_embeds": "ctx"},
              timestep=torch.full((1, 3), 500, dtype=torch.int64), kv_cache_meta=[{}], crossattn_cache_meta=[{}], current_start=48,
              kv_cache_manager="kvm", kv_cache_requests=["r"])
    kw.update(over)
    return kw


def test_wrapper_hands_the_model_the_recorded_keywords():
    from inferix_amd.wan import HipCausVidDiffusionWrapper, HipWanDiffusionWrapper
    m = _RecModel()
    w = HipWanDiffusionWrapper(model=m)
    flow, x0 = w(**_wrapper_kw(cache_start=7))
    assert flow.shape == x0.shape == (1, 3, 4, 2, 2)
    (fa, xa), (fb, xb) = w.forward_pair(_wrapper_kw(), _wrapper_kw(kv_cache_meta=None, kv_start=72, kv_end=144))
    assert fa.shape == xb.shape == (1, 3, 4, 2, 2)
    fc, fu = w.forward_cfg(_wrapper_kw(), _wrapper_kw(kv_cache_manager="neg", kv_start=1, kv_end=2))
    assert fc.shape == fu.shape == (1, 3, 4, 2, 2)
    xa, xb = HipCausVidDiffusionWrapper(model=m).forward_pair(_wrapper_kw(kv_cache_meta=None, kv_start=0, kv_end=72),
                                                             _wrapper_kw(kv_cache_meta=None, kv_start=72, kv_end=144))
    assert xa.shape == xb.shape == (1, 3, 4, 2, 2)
    got = json.loads(json.dumps(m.calls))
    _check("wrapper-keywords", got)


@pytest.mark.parametrize("bad", [dict(kv_cache_meta=None), dict(classify_mode=True), dict(clean_x=torch.zeros(1))])
def test_wrapper_refuses_anything_but_the_kv_cached_inference_call(bad):
    from inferix_amd.wan import HipWanDiffusionWrapper
    w = HipWanDiffusionWrapper(model=_RecModel())
    text = "HipWanDiffusionWrapper implements the KV-cached inference call only"
    with pytest.raises(NotImplementedError) as e:
        w(**_wrapper_kw(**bad))
    assert str(e.value) == text
    for entry in (w.forward_pair, w.forward_cfg):
        for order in ((_wrapper_kw(**bad), _wrapper_kw()), (_wrapper_kw(), _wrapper_kw(kv_cache_manager="neg", **bad))):
            with pytest.raises(NotImplementedError) as e:
                entry(*order)
            assert str(e.value) == text
    assert w.model.calls == []                                               # refused before anything reached the model
    # the CausVid call names its slots instead of a meta list: forward_pair takes it, forward_cfg does not
    slots = _wrapper_kw(kv_cache_meta=None, kv_start=0, kv_end=72)
    w.forward_pair(slots, slots)
    with pytest.raises(NotImplementedError) as e:
        w.forward_cfg(slots, _wrapper_kw(kv_cache_manager="neg"))
    assert str(e.value) == text
    for half in (dict(kv_start=0), dict(kv_end=72)):                         # both slots or none
        with pytest.raises(NotImplementedError):
            w.forward_pair(_wrapper_kw(kv_cache_meta=None, **half), _wrapper_kw())

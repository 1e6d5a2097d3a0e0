#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/unipc_steps.npz and tests/golden/causal_diffusion_tiny.npz: the yardsticks of the
many-step causal sampler (inferix_amd/pipeline/causal_diffusion_inference.py, FlowUniPCSchedule, ifx_cfg_unipc_step).

unipc_steps.npz: the REFERENCE's own `FlowUniPCMultistepScheduler` (models/wan_base/utils/fm_solvers_unipc.py) through
oracle/_refstub.py.  diffusers is not installed, so `register_to_config` is a stub and the object has no `.config`: one is attached by
hand with the constructor's defaults.  At (steps, shift) = (5, 5.0), (8, 5.0), (4, 3.0) the scheduler walks seeded bf16-representable
samples and flows in float64, float32 and bf16; per step the fixture holds the three runs' outputs and the inputs, per schedule the
timesteps and sigmas.  The flow of step i is the same tensor in the three runs (teacher-forced), the sample is each run's own.

causal_diffusion_tiny.npz: the reference's `CausalDiffusionInferencePipeline.inference` on the CPU on the tiny config and seeded
weights of oracle/gen_golden.py.  The class never initialises `kv_cache_meta_pos` / `parallel_config` and hard-codes 30 layers / 1560
tokens: the four attributes are set by hand.  sampling_steps = 5, guidance 3.0, a fake text encoder with distinct embeddings for the
negative prompt.  Case a: 2 blocks of 3 frames, batch 1, text to video; case b: batch 2, one block of `initial_latent` + 1 generated
block.  Per case: inputs, output latents, the integer trace of every generator call on each cache, the first generated block, and
`exact` — the same loop on wan_oracle.generator_forward(attn_impl="math") with two CacheStates and the scheduler in float64.

usage (build container only; the reference tree must exist):  python tools/gen_golden_causal_diffusion.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refstub  # noqa: E402
import wan_oracle as O  # noqa: E402
from fixture_io import GOLDEN_DIR, save_npz, weights_checksum  # noqa: E402

torch.set_grad_enabled(False)
BF = torch.bfloat16
SCHEDULES = [(5, 5.0), (8, 5.0), (4, 3.0)]
SHAPE = (1, 3, 4, 4, 6)                      # [B, F, C, H, W] of the scheduler walk
NEGATIVE = "the negative prompt"
GUIDANCE, SAMPLING_STEPS, SHIFT, NFB = 3.0, 5, 5.0, 3


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def ref_scheduler(unipc_mod, steps, shift):
    s = unipc_mod.FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    s.config = SimpleNamespace(solver_order=2, prediction_type="flow_prediction", predict_x0=True, solver_type="bh2",
                               lower_order_final=True, disable_corrector=[], final_sigmas_type="zero", use_dynamic_shifting=False,
                               thresholding=False, num_train_timesteps=1000, shift=1)
    s.set_timesteps(steps, device="cpu", shift=shift)
    return s


def gen_unipc(unipc_mod):
    fx = {"n_schedules": torch.tensor(len(SCHEDULES)), "schedules": torch.tensor([[s, sh] for s, sh in SCHEDULES], dtype=torch.float64)}
    for k, (steps, shift) in enumerate(SCHEDULES):
        g = torch.Generator().manual_seed(4000 + k)
        x0 = torch.randn(*SHAPE, generator=g).to(BF)
        flows = [torch.randn(*SHAPE, generator=g).to(BF) for _ in range(steps)]
        runs = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32), ("bf16", BF)):
            s = ref_scheduler(unipc_mod, steps, shift)
            x, outs = x0.to(dt), []
            for i, t in enumerate(s.timesteps):
                x = s.step(flows[i].to(dt), t, x, return_dict=False)[0]
                assert x.dtype == dt
                outs.append(x)
            runs[name] = outs
        fx[f"s{k}_timesteps"], fx[f"s{k}_sigmas"] = s.timesteps, s.sigmas
        fx[f"s{k}_sample"] = x0
        for i in range(steps):
            fx[f"s{k}_flow{i}"] = flows[i]
            for name in runs:
                fx[f"s{k}_out{i}_{name}"] = runs[name][i]
        print(f"  schedule {steps} steps, shift {shift}: rel_l2(f32, f64) {[f'{rel_l2(a, b):.2e}' for a, b in zip(runs['f32'], runs['f64'])]}")
        print(f"     rel_l2(bf16, f64) {[f'{rel_l2(a, b):.2e}' for a, b in zip(runs['bf16'], runs['f64'])]}")
    save_npz(os.path.join(GOLDEN_DIR, "unipc_steps.npz"), fx)


class FakeTextEncoder:
    def __init__(self, pos, neg):
        self.pos, self.neg = pos, neg

    def __call__(self, text_prompts):
        return {"prompt_embeds": self.neg if text_prompts[0] == NEGATIVE else self.pos}


def run_reference(cm, unipc_mod, cfg, W, noise, pos, neg, init):
    from gen_golden import build_ref_model
    from inferix.kvcache_manager.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix.models.schedulers.flow_match import FlowMatchScheduler
    from inferix.models.self_forcing.wrapper import WanDiffusionWrapper
    import inferix.pipeline.self_forcing.CausalDiffusionInferencePipeline as mod

    m = build_ref_model(cm, cfg, W)
    w = WanDiffusionWrapper.__new__(WanDiffusionWrapper)
    torch.nn.Module.__init__(w)
    w.model, w.uniform_timestep, w.seq_len, w.parallel_config = m, False, 32760, m.parallel_config
    w.scheduler = FlowMatchScheduler(shift=SHIFT, sigma_min=0.0, extra_one_step=True)
    w.scheduler.set_timesteps(1000, training=True)
    # the prefill hands the wrapper a [B, 1] timestep for a block of 3 frames: its x0 conversion (whose result the pipeline throws
    # away there) broadcasts B sigmas against B * 3 frames, which only works at batch 1.  Give it one sigma per frame instead.
    convert = w._convert_flow_pred_to_x0
    w._convert_flow_pred_to_x0 = lambda flow_pred, xt, timestep: convert(
        flow_pred=flow_pred, xt=xt, timestep=timestep.repeat_interleave(flow_pred.shape[0] // timestep.shape[0]))
    args = SimpleNamespace(num_train_timestep=1000, timestep_shift=SHIFT, guidance_scale=GUIDANCE, negative_prompt=NEGATIVE,
                           num_frame_per_block=NFB, independent_first_frame=False, model_kwargs={})
    vae = SimpleNamespace(decode_to_pixel=lambda latents: latents.float())
    pipe = mod.CausalDiffusionInferencePipeline(args, "cpu", generator=w, text_encoder=FakeTextEncoder(pos, neg), vae=vae)
    pipe.kv_cache_meta_pos, pipe.parallel_config = None, None
    pipe.num_transformer_blocks, pipe.frame_seq_length = cfg.num_layers, cfg.frame_seqlen
    pipe.sampling_steps = SAMPLING_STEPS
    pipe._initialize_sample_scheduler = lambda noise_: ref_scheduler(unipc_mod, pipe.sampling_steps, pipe.shift)
    kvm_pos, kvm_neg = KVCacheManager(device="cpu"), KVCacheManager(device="cpu")
    reqs = [KVCacheRequest(f"req{i}") for i in range(noise.shape[0])]
    trace = {"pos": [], "neg": []}

    def hook(module, a, kw, out):
        meta = kw["kv_cache_meta"][0]
        trace["pos" if kw["kv_cache_manager"] is kvm_pos else "neg"].append(
            [int(kw["current_start"]), int(meta["global_end_index"].item()), int(meta["local_end_index"].item()),
             int(round(float(kw["timestep"].flatten()[0])))])
    h = w.register_forward_hook(hook, with_kwargs=True)
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):     # its per-step prints and tqdm bar
            _, out = pipe.inference(noise=noise, text_prompts=["a prompt"] * noise.shape[0], kv_cache_manager_pos=kvm_pos,
                                    kv_cache_manager_neg=kvm_neg, kv_cache_requests=reqs, initial_latent=init, return_latents=True)
    finally:
        h.remove()
    return out, trace


def run_exact(unipc_mod, cfg, W, noise, pos, neg, init):
    """The same loop with exact attention and the scheduler in float64 (the model takes the latents rounded to bf16, as it does
    everywhere; nothing else of the sampler is rounded)."""
    b, nfr = noise.shape[:2]
    sched = O.FlowMatchSchedule(shift=SHIFT)
    states = [O.CacheState.allocate(cfg, b, BF), O.CacheState.allocate(cfg, b, BF)]
    for st in states:
        st.reset()
    fs = cfg.frame_seqlen
    n_in = init.shape[1] if init is not None else 0
    out = torch.zeros(b, nfr + n_in, *noise.shape[2:], dtype=torch.float64)

    def both(x, t, cur):
        return [O.generator_forward(W, cfg, sched, x.to(BF), list(pe), t, st, cur * fs, "math")[0] for pe, st in zip((pos, neg), states)]
    cur = 0
    for _ in range(n_in // NFB):
        ref = init[:, cur:cur + NFB]
        out[:, cur:cur + NFB] = ref.double()
        both(ref, torch.zeros(b, NFB, dtype=torch.int64), cur)
        cur += NFB
    for _ in range(nfr // NFB):
        x = noise[:, cur - n_in:cur - n_in + NFB].double()
        s = ref_scheduler(unipc_mod, SAMPLING_STEPS, SHIFT)
        for t in s.timesteps:
            fc, fu = both(x, t * torch.ones(b, NFB, dtype=torch.float32), cur)
            flow = fu.double() + GUIDANCE * (fc.double() - fu.double())
            x = s.step(flow, t, x, return_dict=False)[0]
        out[:, cur:cur + NFB] = x
        both(x, torch.zeros(b, NFB, dtype=torch.float32), cur)
        cur += NFB
    return out


def gen_pipeline(cm, unipc_mod):
    cfg = O.tiny_config()
    W = O.init_weights(cfg, seed=0)
    fx = {"weights_checksum": torch.tensor(weights_checksum(W)), "guidance": torch.tensor(GUIDANCE), "shift": torch.tensor(SHIFT),
          "sampling_steps": torch.tensor(SAMPLING_STEPS), "num_frame_per_block": torch.tensor(NFB)}
    for case, batch, blocks, with_init in (("a", 1, 2, False), ("b", 2, 1, True)):
        g = torch.Generator().manual_seed(77 + batch)
        noise = torch.randn(batch, blocks * NFB, 16, cfg.latent_h, cfg.latent_w, generator=g).to(BF)
        pos, neg = torch.zeros(batch, cfg.text_len, cfg.text_dim), torch.zeros(batch, cfg.text_len, cfg.text_dim)
        pos[:, :10] = torch.randn(batch, 10, cfg.text_dim, generator=g)
        neg[:, :6] = torch.randn(batch, 6, cfg.text_dim, generator=g)
        pos, neg = pos.to(BF), neg.to(BF)
        init = torch.randn(batch, NFB, 16, cfg.latent_h, cfg.latent_w, generator=g).to(BF) if with_init else None
        out, trace = run_reference(cm, unipc_mod, cfg, W, noise, pos, neg, init)
        exact = run_exact(unipc_mod, cfg, W, noise, pos, neg, init)
        n_in = NFB if with_init else 0
        first = slice(n_in, n_in + NFB)
        print(f"  case {case}: {len(trace['pos'])} + {len(trace['neg'])} generator forwards; floor rel_l2(reference, exact) = "
              f"{rel_l2(out, exact):.3e} (first block {rel_l2(out[:, first], exact[:, first]):.3e})")
        assert trace["pos"] == trace["neg"]
        fx.update({f"{case}_noise": noise, f"{case}_pos": pos, f"{case}_neg": neg, f"{case}_out": out,
                   f"{case}_exact": exact.float(), f"{case}_first_block": out[:, first].clone(),
                   f"{case}_trace_pos": torch.tensor(trace["pos"]), f"{case}_trace_neg": torch.tensor(trace["neg"])})
        if init is not None:
            fx[f"{case}_initial_latent"] = init
    save_npz(os.path.join(GOLDEN_DIR, "causal_diffusion_tiny.npz"), fx)


def main():
    if not _refstub.available():
        raise SystemExit("reference tree not available: fixtures can only be generated in the build container")
    import importlib
    cm = _refstub.import_hot_path()
    unipc_mod = importlib.import_module("inferix.models.wan_base.utils.fm_solvers_unipc")
    print("unipc_steps.npz")
    gen_unipc(unipc_mod)
    print("causal_diffusion_tiny.npz")
    gen_pipeline(cm, unipc_mod)


if __name__ == "__main__":
    main()

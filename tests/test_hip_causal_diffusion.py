"""GPU: the many-step guided causal sampler (`CausalDiffusionInferencePipeline`: per step one `forward_cfg` + one ifx_cfg_unipc_step
launch) against the reference's own pipeline run on the CPU (tests/golden/causal_diffusion_tiny.npz,
tools/gen_golden_causal_diffusion.py), `forward_cfg` against two sequential `forward` calls, and the outer `SelfForcingPipeline` on a
config without `denoising_step_list`."""
from types import SimpleNamespace

import pytest
import torch
import yaml

import wan_oracle as O
from fixture_io import golden, weights_checksum

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NEGATIVE = "the negative prompt"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def fx():
    return golden("causal_diffusion_tiny.npz")


@pytest.fixture(scope="module")
def tiny():
    cfg = O.tiny_config()
    return cfg, O.init_weights(cfg, seed=0)


def make_pipe(cfg, W, fx, pos, neg, pair):
    from inferix_amd.pipeline import CausalDiffusionInferencePipeline
    from inferix_amd.wan import HipWanDiffusionWrapper
    from test_hip_model import build
    gen = HipWanDiffusionWrapper(model=build(cfg, W), timestep_shift=float(fx["shift"]))
    args = SimpleNamespace(num_train_timestep=1000, timestep_shift=float(fx["shift"]), guidance_scale=float(fx["guidance"]),
                           negative_prompt=NEGATIVE, num_frame_per_block=int(fx["num_frame_per_block"]), independent_first_frame=False,
                           frame_seq_length=cfg.frame_seqlen, kv_cache_tokens=21 * cfg.frame_seqlen, pair_forwards=pair)
    enc = lambda text_prompts: {"prompt_embeds": (neg if text_prompts[0] == NEGATIVE else pos).cuda()}
    pipe = CausalDiffusionInferencePipeline(args, "cuda", generator=gen, text_encoder=enc, vae=None)
    pipe.sampling_steps = int(fx["sampling_steps"])
    return pipe


def run_case(cfg, W, fx, case, pair):
    """-> (output latents on the host, [[current_start, global_end, local_end, timestep], ...] per cache)"""
    from inferix_amd.core import DecodeMode
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    from inferix_amd.schedulers import const_tag
    noise = fx[f"{case}_noise"]
    init = fx.get(f"{case}_initial_latent")
    pipe = make_pipe(cfg, W, fx, fx[f"{case}_pos"], fx[f"{case}_neg"], pair)
    assert pipe._pairing() is pair
    model = pipe.generator.model
    model.index_trace = []
    times = []
    both = pipe._both

    def logged(x, cond, uncond, timestep, *a):
        times.append(int(const_tag(timestep)))          # the host-known scalar of the pipeline's constant timestep tensor
        return both(x, cond, uncond, timestep, *a)
    pipe._both = logged
    out = pipe.inference(noise=noise.cuda(), text_prompts=["a prompt"] * noise.shape[0], kv_cache_manager_pos=KVCacheManager("cuda"),
                         kv_cache_manager_neg=KVCacheManager("cuda"), kv_cache_requests=[KVCacheRequest(f"r{i}") for i in range(noise.shape[0])],
                         initial_latent=None if init is None else init.cuda(), decode_mode=DecodeMode.NO_DECODE)
    tr = model.index_trace                               # layer 0 of every forward in call order: cond, uncond, cond, ...
    assert len(tr) == 2 * len(times)
    trace = {w: [list(tr[2 * i + k]) + [times[i]] for i in range(len(times))] for k, w in enumerate(("pos", "neg"))}
    return out.cpu(), trace


@pytest.fixture(scope="module")
def runs(fx, tiny):
    cfg, W = tiny
    assert weights_checksum(W) == int(fx["weights_checksum"])
    return {(case, pair): run_case(cfg, W, fx, case, pair) for case in ("a", "b") for pair in (True, False)}


@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture_case_through_the_pipeline(fx, runs, case):
    """Integer trace of both caches equal to the reference's; output and first generated block within 1.25 x rel_l2(reference, exact)
    + 5e-4 of `exact` (the project's rollout rule); paired and unpaired forwards bit-identical."""
    out, trace = runs[(case, True)]
    out_u, trace_u = runs[(case, False)]
    assert torch.equal(out, out_u) and trace == trace_u
    assert trace["pos"] == fx[f"{case}_trace_pos"].tolist() and trace["neg"] == fx[f"{case}_trace_neg"].tolist()
    ref, exact = fx[f"{case}_out"], fx[f"{case}_exact"]
    assert out.shape == ref.shape and out.dtype == BF and torch.isfinite(out.float()).all()
    nfb = int(fx["num_frame_per_block"])
    n_in = fx[f"{case}_initial_latent"].shape[1] if f"{case}_initial_latent" in fx else 0
    first = slice(n_in, n_in + nfb)
    assert torch.equal(ref[:, first], fx[f"{case}_first_block"])
    if n_in:
        assert torch.equal(out[:, :n_in], fx[f"{case}_initial_latent"])
    for what, sl in (("output", slice(None)), ("first block", first)):
        floor, mine = rel_l2(ref[:, sl], exact[:, sl]), rel_l2(out[:, sl], exact[:, sl])
        print(f"case {case} {what}: HIP vs exact {mine:.3e}, reference vs exact {floor:.3e}, HIP vs reference {rel_l2(out[:, sl], ref[:, sl]):.3e}")
        assert mine <= 1.25 * floor + 5e-4, (case, what, mine, floor)


def test_forward_cfg_equals_two_sequential_forwards(fx, tiny):
    """Two consecutive guided steps of a block (the first initialises the cross-attention caches) and a clean-context re-run: flows,
    sampled rows of both caches and of the text caches bit for bit, device error word clean."""
    from inferix_amd import hip_ops
    from inferix_amd.kvcache_manager import KVCacheManager, KVCacheRequest
    cfg, W = tiny
    pipe = make_pipe(cfg, W, fx, fx["b_pos"], fx["b_neg"], True)
    noise = fx["b_noise"].cuda()
    B, nf = noise.shape[0], 3
    cond = pipe.text_encoder(text_prompts=["a prompt"] * B)
    uncond = pipe.text_encoder(text_prompts=[NEGATIVE] * B)
    blocks = pipe.generator.model.blocks
    got = {}
    for pair in (False, True):
        kvp, kvn = KVCacheManager("cuda"), KVCacheManager("cuda")
        reqs = [KVCacheRequest(f"r{i}") for i in range(B)]
        pipe._initialize_kv_cache(kvp, kvn, reqs, dtype=BF)
        pipe._initialize_crossattn_cache(kvp, kvn, reqs, dtype=BF)
        flows = []
        for t in (999, 952, 0):
            fc, fu = pipe._both(noise[:, :nf], cond, uncond, pipe._timestep(t, (B, nf), "cuda"), 0, kvp, kvn, reqs, pair)
            assert fc.shape == fu.shape == (B, nf, 16, cfg.latent_h, cfg.latent_w)
            flows += [fc.clone(), fu.clone()]
        torch.cuda.synchronize()
        rows = slice(0, nf * cfg.frame_seqlen, 7)
        caches = [kvm.get_raw(r, name)[:, rows].clone() if name == blk.kv_cache_manager.self_name else kvm.get_raw(r, name).clone()
                  for kvm in (kvp, kvn) for r in reqs for blk in blocks
                  for name in (blk.kv_cache_manager.self_name, blk.kv_cache_manager.cross_name)]
        meta = [(int(m["global_end_index"]), int(m["local_end_index"])) for m in pipe.kv_cache_meta_pos + pipe.kv_cache_meta_neg]
        got[pair] = (flows, caches, meta)
        pipe.clear_cache(kvp, kvn, reqs)
    assert not torch.equal(got[False][0][0], got[False][0][1])                     # the two prompts do give two flows
    for a, b in zip(got[False][0] + got[False][1], got[True][0] + got[True][1]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert got[False][2] == got[True][2] == [(nf * cfg.frame_seqlen,) * 2] * (2 * cfg.num_layers)
    assert hip_ops.device_error(clear=False) == 0
    with pytest.raises(ValueError, match="different cache managers"):
        kv = KVCacheManager("cuda")
        pipe.generator.model.forward_cfg(dict(kv_cache_manager=kv), dict(kv_cache_manager=kv))


class ToyVAE:
    def __init__(self):
        self.model, self.decodes = self, []

    def clear_cache(self):
        pass

    def decode_to_pixel(self, latents, use_cache=True, chunk_size=1):
        self.decodes.append(tuple(latents.shape))
        return torch.tanh(latents[:, :, :3].float()).repeat_interleave(2, dim=-1).repeat_interleave(2, dim=-2)


def test_self_forcing_pipeline_runs_a_config_without_denoising_step_list(tmp_path, tiny):
    from inferix_amd.pipeline import CausalDiffusionInferencePipeline, CausalInferencePipeline, SelfForcingPipeline
    cfg, W = tiny
    conf = dict(num_train_timestep=1000, guidance_scale=3.0, negative_prompt=NEGATIVE, num_frame_per_block=3,
                independent_first_frame=False, timestep_shift=5.0, kv_cache_tokens=21 * cfg.frame_seqlen,
                latent_shape=[cfg.in_dim, cfg.latent_h, cfg.latent_w],
                model_kwargs=dict(patch_size=list(cfg.patch_size), text_len=cfg.text_len, in_dim=cfg.in_dim, dim=cfg.dim,
                                  ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, text_dim=cfg.text_dim, out_dim=cfg.out_dim,
                                  num_heads=cfg.num_heads, num_layers=cfg.num_layers, eps=cfg.eps))
    g = torch.Generator().manual_seed(5)
    pe = {False: torch.randn(1, cfg.text_len, cfg.text_dim, generator=g).to(BF).cuda(),
          True: torch.randn(1, cfg.text_len, cfg.text_dim, generator=g).to(BF).cuda()}
    enc = lambda text_prompts: {"prompt_embeds": pe[text_prompts[0] == NEGATIVE].expand(len(text_prompts), -1, -1)}

    def outer(name, conf):
        path = tmp_path / name
        path.write_text(yaml.safe_dump(conf))
        vae = ToyVAE()
        pipe = SelfForcingPipeline(str(path), text_encoder=enc, vae=vae)
        pipe.pipeline.generator.model.load_state_dict(W)
        return pipe, vae
    pipe, vae = outer("diffusion.yaml", conf)
    assert type(pipe.pipeline) is CausalDiffusionInferencePipeline and pipe._pipeline_type == "causal_diffusion"
    assert pipe.pipeline.sampling_steps == 50 and pipe.pipeline.frame_seq_length == cfg.frame_seqlen
    pipe.pipeline.sampling_steps = 4
    torch.manual_seed(3)
    video = pipe.run_text_to_video(["a prompt"], num_output_frames=6, num_samples=2)
    assert video.shape == (2, 6, 3, 2 * cfg.latent_h, 2 * cfg.latent_w) and torch.isfinite(video).all()
    assert 0.0 <= float(video.min()) and float(video.max()) <= 1.0 and float(video.std()) > 0
    assert vae.decodes == [(2, 6, cfg.in_dim, cfg.latent_h, cfg.latent_w)]
    with pytest.raises(NotImplementedError, match="few-step pipeline"):
        pipe._generate_segment_with_streaming("a prompt", None, None)
    few, _ = outer("few.yaml", dict(conf, denoising_step_list=[1000, 500], warp_denoising_step=True, context_noise=0))
    assert type(few.pipeline) is CausalInferencePipeline and few._pipeline_type == "causal"

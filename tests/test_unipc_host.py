"""CPU: the host side of the many-step causal sampler — `FlowUniPCSchedule` against the reference's own scheduler runs
(tests/golden/unipc_steps.npz, tools/gen_golden_causal_diffusion.py), the properties of its coefficient table, the wiring of
ifx_cfg_unipc_step through header, bindings and library, the import paths, the refusals and `SelfForcingPipeline`'s class selection."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from fixture_io import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def fx():
    return golden("unipc_steps.npz")


def _schedules(fx):
    return [(k, int(s), float(sh)) for k, (s, sh) in enumerate(fx["schedules"].tolist())]


def _schedule(steps, shift):
    from inferix_amd.schedulers import FlowUniPCSchedule
    s = FlowUniPCSchedule(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    s.set_timesteps(steps, device="cpu", shift=shift)
    return s


def test_solver_parity_with_the_reference_float64_run(fx):
    """The closed-form table in float64 on the fixture's inputs: at every step of the three schedules within 2 x the distance of the
    reference's own float32 run from its float64 run (two evaluations of one formula; measured ratios up to 1.16)."""
    assert [(s, sh) for _, s, sh in _schedules(fx)] == [(5, 5.0), (8, 5.0), (4, 3.0)]
    for k, steps, shift in _schedules(fx):
        s = _schedule(steps, shift)
        x = fx[f"s{k}_sample"].double()
        for i, t in enumerate(s.timesteps):
            x = s.step(fx[f"s{k}_flow{i}"].double(), t, x, return_dict=False)[0]
            assert x.dtype == torch.float64
            ref64, ref32 = fx[f"s{k}_out{i}_f64"], fx[f"s{k}_out{i}_f32"]
            mine, floor = rel_l2(x, ref64), rel_l2(ref32, ref64)
            print(f"schedule {k} step {i}: restatement {mine:.3e}, reference float32 {floor:.3e}, ratio {mine / floor:.2f}")
            assert mine <= 2.0 * floor, (k, i, mine, floor)


def test_bf16_host_step_stays_in_the_tensors_dtype(fx):
    k, steps, shift = _schedules(fx)[0]
    s = _schedule(steps, shift)
    x = fx[f"s{k}_sample"]
    for i, t in enumerate(s.timesteps):
        x = s.step(fx[f"s{k}_flow{i}"], t, x, return_dict=False)[0]
        assert x.dtype == torch.bfloat16 and rel_l2(x, fx[f"s{k}_out{i}_f64"]) < 2e-2
    with pytest.raises(IndexError):
        s.step(fx[f"s{k}_flow0"], s.timesteps[-1], x)


def test_table_properties(fx):
    for k, steps, shift in _schedules(fx):
        s = _schedule(steps, shift)
        assert s.timesteps.dtype == torch.int64 and torch.equal(s.timesteps, fx[f"s{k}_timesteps"])
        assert s.sigmas.dtype == torch.float32 and torch.equal(s.sigmas, fx[f"s{k}_sigmas"]) and float(s.sigmas[-1]) == 0.0
        table = s.coefficients()
        assert len(table) == steps and table is s.coefficients() and table is _schedule(steps, shift).coefficients()     # cached per (steps, shift)
        assert [c.predictor_order for c in table] == [1] + [2] * (steps - 2) + [1]
        assert [c.use_corrector for c in table] == [False] + [True] * (steps - 1)
        assert [c.corrector_order for c in table[1:]] == [c.predictor_order for c in table[:-1]]
        for c in table:
            assert all(isinstance(v, (float, int, bool)) and math.isfinite(v) for v in c), c
        last = table[-1]
        assert (last.p_x, last.p_m, last.p_d) == (0.0, 1.0, 0.0)                 # sigma_next = 0: x_next = m_t
        assert table[0].c_last == table[0].c_dt == 0.0 and all(c.p_d != 0.0 for c in table[1:-1])
        assert [c.sigma for c in table] == [float(v) for v in s.sigmas[:-1].double()]
    other = _schedule(5, 3.0).coefficients()
    assert other is not _schedule(5, 5.0).coefficients() and other[1].p_x != _schedule(5, 5.0).coefficients()[1].p_x


def test_step_needs_set_timesteps_and_a_timestep_on_the_grid():
    from inferix_amd.schedulers import FlowUniPCSchedule
    s = FlowUniPCSchedule()
    x = torch.zeros(1, 1, 1, 2, 2)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(x, 999, x)
    s.set_timesteps(5, shift=5.0)
    with pytest.raises(ValueError, match="not on the grid"):
        s.step(x, 1, x)
    with pytest.raises(NotImplementedError):
        FlowUniPCSchedule(use_dynamic_shifting=True)


def test_cfg_unipc_step_is_exported_bound_and_refuses_bad_arguments():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert re.search(r"\bint\s+ifx_cfg_unipc_step\s*\(const ifx_cfg_unipc_step_desc\*", hdr)
    assert int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1)) == 7 == _hip.ABI_MINOR
    assert _hip.SIGNATURES["ifx_cfg_unipc_step"] == (C.c_int, [C.POINTER(_hip.CfgUnipcStepDesc), C.c_void_p])
    lib = _hip.load()
    assert (lib.ifx_version() >> 8) & 255 == 7
    # the struct of the header, field by field: 2 pointers, 6 strides, 7 pointers, 4 + 9 + 3 four-byte scalars
    D = _hip.CfgUnipcStepDesc
    assert C.sizeof(D) == 16 + 48 + 56 + 64 and D.x.offset == 64 and D.batch.offset == 120 and D.guidance.offset == 136
    assert D.use_corrector.offset == 172
    makefile = open(os.path.join(ROOT, "inferix_amd", "csrc", "Makefile")).read()
    assert "ifx_sampler.hip" in makefile and os.path.exists(os.path.join(ROOT, "inferix_amd", "csrc", "ifx_sampler.hip"))
    from inferix_amd import hip_ops
    assert callable(hip_ops.cfg_unipc_step)
    # refusals happen on the host, before any launch
    assert lib.ifx_cfg_unipc_step(None, None) == -1
    d = D()
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"null" in lib.ifx_last_error()
    buf = (C.c_uint16 * 64)()
    base = C.addressof(buf)
    for f in ("flow_cond", "flow_uncond", "x", "x_next", "last_out", "m_out"):
        setattr(d, f, base)
    d.batch, d.frames, d.channels, d.plane = 1, 1, 1, 8
    d.corrector_order = d.predictor_order = 3
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"order" in lib.ifx_last_error()
    d.corrector_order, d.predictor_order, d.use_corrector = 1, 1, 1
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"needs last_sample and m1" in lib.ifx_last_error()
    d.use_corrector, d.predictor_order = 0, 2
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"needs m1" in lib.ifx_last_error()
    d.predictor_order, d.x = 1, base + 1
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"2-byte aligned" in lib.ifx_last_error()
    d.x, d.channels = base, 2
    d.flow_cond_stride[2], d.flow_uncond_stride[2] = 4, 8
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"smaller than a plane" in lib.ifx_last_error()
    d.plane = 0
    assert lib.ifx_cfg_unipc_step(C.byref(d), None) == -1 and b"bad geometry" in lib.ifx_last_error()


def test_wrapper_refuses_host_tensors_and_wrong_layouts():
    from inferix_amd import _hip, hip_ops
    from inferix_amd.schedulers import FlowUniPCSchedule
    s = FlowUniPCSchedule()
    s.set_timesteps(5, shift=5.0)
    c = s.coefficients()[0]
    x = torch.zeros(1, 1, 2, 2, 4, dtype=torch.bfloat16)
    with pytest.raises(_hip.HipKernelError, match="GPU only"):
        hip_ops.cfg_unipc_step(x, x, x, None, None, None, c, 1.0, x, x, x)
    with pytest.raises(ValueError, match=r"\[B, F, C, H, W\]"):
        hip_ops.cfg_unipc_step(x[0], x[0], x[0], None, None, None, c, 1.0, x[0], x[0], x[0])


def test_import_paths_resolve():
    from inferix.models.wan_base import FlowUniPCMultistepScheduler
    from inferix.models.wan_base.utils.fm_solvers_unipc import FlowUniPCMultistepScheduler as F2
    from inferix.pipeline.self_forcing.CausalDiffusionInferencePipeline import CausalDiffusionInferencePipeline
    import inferix_amd.pipeline as P
    from inferix_amd.schedulers import FlowUniPCSchedule
    assert FlowUniPCMultistepScheduler is F2 is FlowUniPCSchedule
    assert CausalDiffusionInferencePipeline is P.CausalDiffusionInferencePipeline
    s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    s.set_timesteps(50, device="cpu", shift=5.0)
    assert len(s.timesteps) == 50 and len(s.sigmas) == 51


def _fake_generator(world_size=1):
    model = SimpleNamespace(local_attn_size=-1, num_layers=2, patch_size=(1, 2, 2), text_len=16, blocks=[])
    sched = SimpleNamespace(timesteps=torch.arange(1000, 0, -1, dtype=torch.float32))
    return SimpleNamespace(model=model, parallel_config=SimpleNamespace(world_size=world_size, rank=0, local_rank=0),
                           get_scheduler=lambda: sched, forward_cfg=None, forward_pair=None)


def _args(**over):
    a = dict(num_train_timestep=1000, timestep_shift=5.0, guidance_scale=3.0, negative_prompt="bad", num_frame_per_block=3,
             independent_first_frame=False, frame_seq_length=24)
    a.update(over)
    return SimpleNamespace(**a)


def test_refusals_name_themselves():
    from inferix_amd.pipeline import CausalDiffusionInferencePipeline
    pipe = CausalDiffusionInferencePipeline(_args(), "cpu", generator=_fake_generator())
    assert (pipe.sampling_steps, pipe.sample_solver, pipe.shift, pipe.num_transformer_blocks, pipe.frame_seq_length) == \
        (50, "unipc", 5.0, 2, 24)
    assert pipe.kv_cache_meta_pos is None and pipe.parallel_config.world_size == 1
    s = pipe._initialize_sample_scheduler(torch.zeros(1))
    assert len(s.timesteps) == 50 and s.step_index is None
    pipe.sample_solver = "dpm++"
    with pytest.raises(NotImplementedError, match=r"dpm\+\+"):
        pipe._initialize_sample_scheduler(torch.zeros(1))
    pipe.sample_solver = "euler"
    with pytest.raises(NotImplementedError, match="only 'unipc' is built"):
        pipe._initialize_sample_scheduler(torch.zeros(1))
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        CausalDiffusionInferencePipeline(_args(), "cpu", generator=_fake_generator(world_size=2))
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        CausalDiffusionInferencePipeline(_args(), "cpu", generator=_fake_generator(), parallel_config=SimpleNamespace(world_size=4))
    # the outer class: neither a step list nor the guided sampler's settings names no pipeline that is built
    from inferix_amd.pipeline import SelfForcingPipeline
    with pytest.raises(NotImplementedError, match="needs guidance_scale and negative_prompt"):
        SelfForcingPipeline({"model_kwargs": {}})
    with pytest.raises(NotImplementedError, match="needs negative_prompt;"):
        SelfForcingPipeline({"model_kwargs": {}, "guidance_scale": 3.0})


def test_self_forcing_pipeline_selects_the_inner_class_from_the_config():
    """`_initialize_pipeline` on an object built without the constructor (which needs a GPU): with a `denoising_step_list` the few-step
    pipeline, without one the many-step sampler, as the reference's pipeline.py:67."""
    from inferix_amd.pipeline import CausalDiffusionInferencePipeline, CausalInferencePipeline, SelfForcingPipeline

    def outer(config):
        p = object.__new__(SelfForcingPipeline)
        p.config, p.device, p.latent_shape, p._profiler = config, torch.device("cpu"), [16, 8, 12], None
        p.parallel_config = SimpleNamespace(world_size=1, rank=0, local_rank=0)
        p._initialize_pipeline(generator=_fake_generator())
        return p
    few = outer(_args(denoising_step_list=[1000, 500]))
    assert type(few.pipeline) is CausalInferencePipeline and few._pipeline_type == "causal"
    many = outer(_args())
    assert type(many.pipeline) is CausalDiffusionInferencePipeline and many._pipeline_type == "causal_diffusion"
    assert many._init_model() is many.pipeline and many.pipeline.frame_seq_length == 24
    with pytest.raises(NotImplementedError, match="streaming generation is built for the few-step pipeline"):
        many._generate_segment_with_streaming("a prompt", None, None)

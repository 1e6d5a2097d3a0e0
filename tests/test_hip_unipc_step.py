"""GPU: `ifx_cfg_unipc_step` (guidance mix + x0 conversion + UniC corrector + UniP predictor of one sampling step in one launch) against
the float64 evaluation of its own linear form, taken with the fp32 coefficient values the kernel was handed.

The bound on all three outputs is derived, not measured: |out - y64| <= 1/2 ulp_bf16(y64) + 16 * 2^-24 * S, S the same form with every
coefficient and input replaced by its absolute value — one rounding to bf16 per output, and at most sixteen fp32 roundings (the
kernel's FMAs make thirteen from the inputs to x_next) on partial sums bounded by S.  Against the reference's operator chain
(tests/golden/unipc_steps.npz): the fused step must not be further from the float64 run than the reference's own bf16 run."""
import pytest
import torch

from fixture_io import golden

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def table(steps=8, shift=5.0):
    from inferix_amd.schedulers import FlowUniPCSchedule
    s = FlowUniPCSchedule()
    s.set_timesteps(steps, shift=shift)
    return s.coefficients()


class Padded:
    """A bf16 tensor of `shape` that starts `offset` elements into a NaN-filled allocation (256-byte aligned by torch) with NaN behind
    it as well; `.t` is the tensor, `intact()` says whether the padding still holds what it held."""
    def __init__(self, shape, offset, gen, fill=True, pad=24):
        n = 1
        for d in shape:
            n *= d
        self.whole = torch.full((offset + n + pad,), float("nan"), dtype=BF, device=DEV)
        self.lo, self.hi = offset, offset + n
        self.t = self.whole[self.lo:self.hi].view(*shape)
        if fill:
            self.t.copy_(torch.randn(*shape, generator=gen).to(BF))

    def intact(self):
        return bool(torch.isnan(self.whole[:self.lo]).all()) and bool(torch.isnan(self.whole[self.hi:]).all())


def make_inputs(geom, offsets, permuted, seed):
    """The six inputs and three outputs: the flows as `[B, C, F, H, W]` blocks viewed `[B, F, C, H, W]` (what the model hands over) or
    contiguous; everything at its own offset from a 16-byte boundary."""
    B, Fn, Cn, H, W = geom
    g = torch.Generator().manual_seed(seed)
    o = dict(zip(("fc", "fu", "x", "last", "m1", "m2", "x_next", "last_out", "m_out"), offsets))
    bufs = {}
    for name in ("fc", "fu"):
        p = Padded((B, Cn, Fn, H, W) if permuted else (B, Fn, Cn, H, W), o[name], g)
        bufs[name] = (p, p.t.permute(0, 2, 1, 3, 4) if permuted else p.t)
    for name in ("x", "last", "m1", "m2"):
        p = Padded((B, Fn, Cn, H, W), o[name], g)
        bufs[name] = (p, p.t)
    for name in ("x_next", "last_out", "m_out"):
        p = Padded((B, Fn, Cn, H, W), o[name], g, fill=False)
        bufs[name] = (p, p.t)
    return bufs


def linear_form(c, guidance, fc, fu, x, last, m1, m2):
    """(y64, S) of the three outputs in float64, with the fp32 values of the coefficients the kernel received."""
    g, sg = f32(guidance), f32(c.sigma)
    fc, fu, x, last, m1, m2 = (t.double().cpu() for t in (fc, fu, x, last, m1, m2))
    flow, flow_a = fu + g * (fc - fu), fu.abs() + abs(g) * (fc.abs() + fu.abs())
    m_t, m_a = x - sg * flow, x.abs() + abs(sg) * flow_a
    if c.use_corrector:
        cl, c1, cd, ct = f32(c.c_last), f32(c.c_m1), f32(c.c_d1), f32(c.c_dt)
        x_c = cl * last + c1 * m1 + ct * (m_t - m1)
        xc_a = abs(cl) * last.abs() + abs(c1) * m1.abs() + abs(ct) * (m_a + m1.abs())
        if c.corrector_order == 2:
            x_c, xc_a = x_c + cd * (m2 - m1), xc_a + abs(cd) * (m2.abs() + m1.abs())
    else:
        x_c, xc_a = x, x.abs()
    px, pm, pd = f32(c.p_x), f32(c.p_m), f32(c.p_d)
    x_n, xn_a = px * x_c + pm * m_t, abs(px) * xc_a + abs(pm) * m_a
    if c.predictor_order == 2:
        x_n, xn_a = x_n + pd * (m1 - m_t), xn_a + abs(pd) * (m1.abs() + m_a)
    return (x_n, x_c, m_t), (xn_a, xc_a, m_a)


def ulp_bf16(y):
    _, e = torch.frexp(y.abs().clamp_min(2.0 ** -126))       # |y| = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e - 8)
    return torch.ldexp(torch.ones_like(y), e - 8)


def check(outs, y64, S, what):
    for name, out, y, s in zip(("x_next", "last_out", "m_out"), outs, y64, S):
        err = (out.double().cpu() - y).abs()
        bound = 0.5 * ulp_bf16(y) + 16 * 2.0 ** -24 * s
        worst = float((err / bound).max())
        assert worst <= 1.0, f"{what}: {name} at {worst:.3f} of the bound (max error {float(err.max()):.3e})"


def launch(c, guidance, b):
    from inferix_amd import hip_ops
    t = {k: v[1] for k, v in b.items()}
    hip_ops.cfg_unipc_step(t["fc"], t["fu"], t["x"], t["last"], t["m1"], t["m2"], c, guidance, t["x_next"], t["last_out"], t["m_out"])
    torch.cuda.synchronize()
    return t


# [B, F, C, H, W]: H W of 1, 6, 8 and 60 (tail only, vector only, vectors and a tail), 1 .. 96 planes (several workgroups)
GEOMS = [(1, 1, 1, 1, 1), (1, 2, 3, 2, 3), (1, 3, 4, 2, 4), (2, 3, 16, 6, 10), (1, 1, 2, 6, 10)]
OFFSETS = {"aligned": (8,) * 9,                                   # every plane start with P % 8 == 0 on a 16-byte boundary
           "shifted": (3,) * 9,                                   # 6 bytes off, all alike: a scalar head, then 16-byte groups
           "mixed": (8, 3, 8, 5, 8, 8, 1, 8, 2)}                  # offsets disagree: the 2-byte path throughout
STEPS = (0, 1, 3, 7)                                              # no corrector / corrector 1 + predictor 2 / middle / sigma_next = 0


@pytest.mark.parametrize("offsets", list(OFFSETS))
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_every_step_kind_guidance_and_layout_within_the_derived_bound(geom, offsets):
    tab = table()
    assert (tab[0].use_corrector, tab[1].corrector_order, tab[1].predictor_order, tab[3].corrector_order, tab[7].p_x) == \
        (False, 1, 2, 2, 0.0)
    seed = 0
    for step in STEPS:
        for guidance in (0.0, 1.0, 3.0):
            for permuted in (True, False):
                seed += 1
                b = make_inputs(geom, OFFSETS[offsets], permuted, seed)
                before = {k: b[k][1].clone() for k in ("fc", "fu", "x", "last", "m1", "m2")}
                t = launch(tab[step], guidance, b)
                y64, S = linear_form(tab[step], guidance, *(before[k] for k in ("fc", "fu", "x", "last", "m1", "m2")))
                check((t["x_next"], t["last_out"], t["m_out"]), y64, S, f"step {step} guidance {guidance} permuted {permuted}")
                for k, (p, _) in b.items():
                    assert p.intact(), f"{k}: padding written (step {step})"
                for k, v in before.items():
                    assert torch.equal(v, b[k][1]), f"{k}: input written"


@pytest.mark.parametrize("step", STEPS)
def test_aliased_outputs_equal_the_out_of_place_result(step):
    """x_next on x, last_out on last_sample, m_out on the slot of m2 — one at a time and all three together."""
    from inferix_amd import hip_ops
    tab = table()
    for geom in ((2, 3, 16, 6, 10), (1, 2, 3, 2, 3)):
        b = make_inputs(geom, OFFSETS["aligned"], True, 100 + step)
        ref = {k: v.clone() for k, v in launch(tab[step], 3.0, b).items()}
        for alias in (("x",), ("last",), ("m2",), ("x", "last", "m2")):
            t = {k: v[1].clone() if k in ("x", "last", "m1", "m2") else v[1] for k, v in b.items()}
            outs = dict(x_next=t["x"] if "x" in alias else torch.empty_like(t["x"]),
                        last_out=t["last"] if "last" in alias else torch.empty_like(t["x"]),
                        m_out=t["m2"] if "m2" in alias else torch.empty_like(t["x"]))
            hip_ops.cfg_unipc_step(t["fc"], t["fu"], t["x"], t["last"], t["m1"], t["m2"], tab[step], 3.0, **outs)
            torch.cuda.synchronize()
            for k in outs:
                assert torch.equal(outs[k], ref[k]), (geom, alias, k)


def test_optional_slots_and_wrapper_refusals():
    from inferix_amd import hip_ops
    tab = table()
    b = make_inputs((1, 2, 3, 2, 4), OFFSETS["aligned"], False, 7)
    t = {k: v[1] for k, v in b.items()}
    ref = {k: v.clone() for k, v in launch(tab[0], 3.0, b).items()}
    outs = [torch.empty_like(t["x"]) for _ in range(3)]
    hip_ops.cfg_unipc_step(t["fc"], t["fu"], t["x"], None, None, None, tab[0], 3.0, *outs)          # the first step reads no history
    torch.cuda.synchronize()
    assert all(torch.equal(o, ref[k]) for o, k in zip(outs, ("x_next", "last_out", "m_out")))
    assert torch.equal(outs[1], t["x"])                                                               # no corrector: x_c = x
    with pytest.raises(ValueError, match="reads it"):
        hip_ops.cfg_unipc_step(t["fc"], t["fu"], t["x"], None, t["m1"], None, tab[1], 3.0, *outs)
    with pytest.raises(ValueError, match="contiguous"):
        strided = t["x"].permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)                   # the flows' layout: not for x
        hip_ops.cfg_unipc_step(t["fc"], t["fu"], strided, None, None, None, tab[0], 3.0, *outs)
    with pytest.raises(ValueError, match="contiguous"):
        hip_ops.cfg_unipc_step(t["fc"].transpose(3, 4).contiguous().transpose(3, 4), t["fu"], t["x"], None, None, None, tab[0], 3.0, *outs)
    with pytest.raises(TypeError):
        hip_ops.cfg_unipc_step(t["fc"].float(), t["fu"], t["x"], None, None, None, tab[0], 3.0, *outs)
    assert hip_ops.device_error(clear=False) == 0


def test_fused_chain_is_no_further_from_float64_than_the_reference_bf16_chain():
    """The fixture's samples and flows through `FlowUniPCSchedule.step` on the device (its own chain: last_sample and the history ring
    are the kernel's outputs), one step at a time: at every step rel_l2(HIP, reference float64 run) <= rel_l2(reference bf16 run,
    reference float64 run).  The bf16 run rounds after every operator, the fused step once per output."""
    from inferix_amd.schedulers import FlowUniPCSchedule
    fx = golden("unipc_steps.npz")
    for k, (steps, shift) in enumerate(fx["schedules"].tolist()):
        s = FlowUniPCSchedule(num_train_timesteps=1000, shift=1)
        s.set_timesteps(int(steps), device="cpu", shift=shift)
        x0 = fx[f"s{k}_sample"].to(DEV)
        x = x0
        for i, t in enumerate(s.timesteps.tolist()):
            flow = fx[f"s{k}_flow{i}"].to(DEV)
            if i % 2:                                  # the model's layout on odd steps, a contiguous flow on even ones
                flow = flow.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
            x = s.step(flow, t, x, return_dict=False)[0]
            ref64 = fx[f"s{k}_out{i}_f64"]
            mine, theirs = rel_l2(x.cpu(), ref64), rel_l2(fx[f"s{k}_out{i}_bf16"], ref64)
            print(f"schedule {k} step {i}: fused {mine:.3e}, reference bf16 chain {theirs:.3e}")
            assert x.dtype == BF and mine <= theirs, (k, i, mine, theirs)
        assert torch.equal(x0.cpu(), fx[f"s{k}_sample"])           # the caller's first sample is never written
        # a second block on the same object reuses the buffers and gives the same bits
        s.set_timesteps(int(steps), device="cpu", shift=shift)
        y = x0
        for i, t in enumerate(s.timesteps.tolist()):
            y = s.step(fx[f"s{k}_flow{i}"].to(DEV), t, y, return_dict=False)[0]
        assert torch.equal(y, x)


def test_guided_step_on_the_device_matches_the_host_step_in_float64():
    """`step_cfg` with two flows: the device launch against the host path of the same object in float64, a whole block."""
    from inferix_amd.schedulers import FlowUniPCSchedule
    g = torch.Generator().manual_seed(11)
    shape = (2, 3, 16, 6, 10)
    x0 = torch.randn(*shape, generator=g).to(BF)
    flows = [(torch.randn(*shape, generator=g).to(BF), torch.randn(*shape, generator=g).to(BF)) for _ in range(5)]
    dev, host = FlowUniPCSchedule(), FlowUniPCSchedule()
    dev.set_timesteps(5, shift=5.0)
    host.set_timesteps(5, shift=5.0)
    xd, xh = x0.to(DEV)[:, :], x0.double()
    for (fc, fu), t in zip(flows, dev.timesteps.tolist()):
        xd = dev.step_cfg(fc.to(DEV), fu.to(DEV), 3.0, t, xd)[0]
        xh = host.step_cfg(fc.double(), fu.double(), 3.0, t, xh)[0]
    assert rel_l2(xd.cpu(), xh) < 1e-2 and dev.step_index == host.step_index == 5

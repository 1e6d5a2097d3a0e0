"""GPU parity of ifx_conv.hip at its own branch points (cases and references: conv_cases.py; that the bars used here can fail:
test_conv_cases_oracle.py): every conv instantiation against torch at the smallest shape that reaches it — channel counts off the
8-channel vector path, ragged and multiple channel tiles, 16 frames per call, the shortest K loops, zero frames in every layout — the
persistent kernel with more tiles than workgroups, the in-place residual the decoder relies on, frame strides with gaps behind canaries,
and ifx_rmsnorm_cl on every instantiation a channel count in [8, 512] selects.

Each comparison prints `CONVEDGE|section|what|worst element error / its bound|mismatch fraction / its cap|rel L2 / its bound` before it
asserts.  The bars are those of test_hip_vae.test_conv3d_cl_against_torch and test_rmsnorm_cl."""
import ctypes as C

import pytest
import torch

import conv_cases as K
from util import assert_bf16_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def bits(t):
    return t.contiguous().view(torch.int16)


def judge(section, what, got, ref, **bars):
    worst, frac, rel = K.parity_figures(got, ref, bars["max_ulp"], bars["floor"])
    print(f"CONVEDGE|{section}|{what}|{worst:.4f}|{frac / 0.02:.4f}|{rel / 1e-3:.4f}")
    assert_bf16_parity(got, ref, what=what, **bars)          # (default caps: 2 % of elements may differ, rel L2 1e-3)


def launch(ops, o, planar, variant=0, y=None, out_slots=None, residual="own"):
    """One hip_ops.conv3d_cl call on the operands of conv_cases.build; returns (y, out_slots).  y defaults to t + 1 zeroed slots."""
    c = o.case
    buf = o.buf.cuda()
    xin = ops.to_planar(buf) if planar else buf
    out_slots = o.out_slots if out_slots is None else out_slots
    if y is None:
        y = torch.zeros(c.t + 1, o.ho, o.wo, c.cout, dtype=BF, device="cuda")
    if isinstance(residual, str):
        residual = o.residual.cuda() if o.residual is not None else None
    ops.set_option("conv_variant", variant)
    try:
        ops.conv3d_cl(xin, o.slots, o.wp.cuda(), o.b.cuda() if o.b is not None else None, kt=c.kt, ks=c.ks, y=y, out_slots=out_slots,
                      upsample=bool(c.ups), residual=residual)
    finally:
        ops.set_option("conv_variant", 0)
    return y, out_slots


def against_torch(ops, section, case, planar):
    """The case under each of its conv_variant settings: against torch, unnamed slot untouched, and the variants bit for bit."""
    o = K.build(case, K.SEED, planar)
    outs = []
    for variant in case.variants:
        y, out_slots = launch(ops, o, planar, variant)
        got = torch.stack([y[s] for s in out_slots]).cpu()
        judge(section, f"{case.name} planar{int(planar)} variant{variant} {K.plan_row(case.kt, case.ks, case.ups, case.cout, variant)}",
              got, o.ref, **K.conv_bars(case))
        untouched = [s for s in range(case.t + 1) if s not in out_slots]
        assert untouched and all(float(y[s].abs().max()) == 0.0 for s in untouched)
        outs.append(y)
    if len(outs) == 2:
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"{case.name}: ping-pong and lock-step conv kernels differ"
    return outs[0]


# ---- A: every instantiation against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("case", K.CONV_CASES, ids=lambda c: c.name)
def test_every_instantiation_against_torch(ops, case, planar):
    against_torch(ops, "A", case, planar)


# ---- B: more tiles than workgroups in the persistent kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("ups", [0, 1])
@pytest.mark.parametrize("width", ["rule", "named"])
def test_persistent_kernel_with_more_tiles_than_workgroups(ops, width, ups):
    """conv_pp_kernel keeps its request stream running across the tiles of one workgroup: here some workgroups of every XCD take a second
    tile and others do not.  "rule": the narrowest such frame for this part's CU count; "named": 24 x 390 (336 tiles)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = K.overflow_case(cus, ups) if width == "rule" else K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, ups)
    row = K.plan_row(case.kt, case.ks, case.ups, case.cout, 0)
    total = K.plan_tiles(case.h << ups, case.w << ups, case.cout, case.t)[3]
    grid = K.plan_grid(row, total, cus)
    assert row == f"pp::conv_pp_kernel<96, {ups}>" and grid == 8 * (cus // 8), (row, grid, cus)
    assert total > grid and total % grid != 0 and -(-total // 8) > cus // 8, f"{total} tiles on {grid} workgroups: no workgroup takes a second tile"
    case = case._replace(variants=(0, 1))
    against_torch(ops, "B", case, False)


# ---- C: in place ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("case", K.INPLACE_CASES, ids=lambda c: c.name)
def test_in_place_residual_equals_out_of_place(ops, case, planar):
    """HipWanVAE._res passes y = residual: every output element is produced by the thread that read that element of the residual."""
    o = K.build(case, K.SEED, planar)
    slots = list(range(case.t))
    for variant in (0, 1) if K.plan_row(case.kt, case.ks, case.ups, case.cout, 0).startswith("pp::") else (0,):
        apart = torch.zeros(case.t, o.ho, o.wo, case.cout, dtype=BF, device="cuda")
        launch(ops, o, planar, variant, y=apart, out_slots=slots)
        judge("C", f"{case.name} planar{int(planar)} variant{variant} out of place", apart.cpu(), o.ref, **K.conv_bars(case))
        same = o.residual.cuda().clone()
        launch(ops, o, planar, variant, y=same, out_slots=slots, residual=same)
        assert torch.equal(bits(same), bits(apart)), f"{case.name} variant {variant}: the in-place launch differs"


# ---- D: strided frames with canaries --------------------------------------------------------------------------------------------------
GAP = 64          # elements between frames (a multiple of 8: the alignment contract of ifx_conv3d_desc)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("case", K.STRIDED_CASES, ids=lambda c: c.name)
def test_frame_strides_with_gaps_behind_canaries(ops, case, planar):
    """in_frame_stride / out_frame_stride = frame + 64 elements: NaN between the input frames, 7.0 between the output frames and in two
    slots that are not named.  The same bits as the dense launch, every sentinel alive, nothing NaN."""
    from inferix_amd import _hip
    o = K.build(case, K.SEED, planar)
    dense = against_torch(ops, "D", case, planar)
    in_frame, out_frame = case.h * case.w * case.cin, o.ho * o.wo * case.cout
    n_phys = o.buf.shape[0]
    buf = o.buf.cuda()
    frames = (ops.to_planar(buf) if planar else buf).reshape(n_phys, in_frame)
    x = torch.full((n_phys, in_frame + GAP), float("nan"), dtype=BF, device="cuda")
    x[:, :in_frame] = frames
    n_out = case.t + 2
    out_slots = list(range(1, case.t + 1))                   # slots 0 and t + 1 are not named
    y = torch.full((n_out, out_frame + GAP), 7.0, dtype=BF, device="cuda")
    w, b = o.wp.cuda(), o.b.cuda() if o.b is not None else None
    res = o.residual.cuda() if o.residual is not None else None
    zero = torch.zeros(256, dtype=torch.uint8, device="cuda")
    ins, outs = (C.c_int32 * len(o.slots))(*o.slots), (C.c_int32 * case.t)(*out_slots)
    assert max(o.slots) < n_phys and max(out_slots) < n_out and x.is_contiguous() and y.is_contiguous()
    for variant in case.variants:
        y.fill_(7.0)
        d = _hip.Conv3dDesc(x.data_ptr(), in_frame + GAP, ins, case.h, case.w, case.cin, case.ups, w.data_ptr(),
                            b.data_ptr() if b is not None else None, case.kt, case.ks, y.data_ptr(), out_frame + GAP, outs, case.cout,
                            case.t, res.data_ptr() if res is not None else None, zero.data_ptr(), 1 if planar else 0)
        ops.set_option("conv_variant", variant)
        try:
            _hip.check(_hip.load().ifx_conv3d_cl(C.byref(d), torch.cuda.current_stream().cuda_stream), "ifx_conv3d_cl")
        finally:
            ops.set_option("conv_variant", 0)
        assert not torch.isnan(y.float()).any(), f"{case.name}: a gap between input frames was read"
        got = y[out_slots, :out_frame].reshape(case.t, o.ho, o.wo, case.cout)
        want = torch.stack([dense[s] for s in o.out_slots])
        assert torch.equal(bits(got), bits(want)), f"{case.name} variant {variant}: strided and dense launches differ"
        assert float((y[:, out_frame:].float() - 7.0).abs().max()) == 0.0, f"{case.name}: a gap behind an output frame was written"
        assert float((y[[0, n_out - 1]].float() - 7.0).abs().max()) == 0.0, f"{case.name}: a slot that was not named was written"
        print(f"CONVEDGE|D|{case.name} planar{int(planar)} variant{variant} strided = dense, canaries alive|0.0000|0.0000|0.0000")


# ---- E: the alignment contract is a host decision (every refusal is pinned without a GPU: test_cabi_and_host.CONV_PLAN_RECORDED) ----------
def test_misaligned_frames_are_refused_before_any_launch(ops):
    from inferix_amd import _hip
    o = K.build(K.CASE["cl128x3-cout200"], K.SEED, False)
    c = o.case
    x, w, res = o.buf.cuda(), o.wp.cuda(), o.residual.cuda()
    y = torch.full((c.t, o.ho, o.wo, c.cout), 7.0, dtype=BF, device="cuda")
    zero = torch.zeros(256, dtype=torch.uint8, device="cuda")
    ins, outs = (C.c_int32 * len(o.slots))(*o.slots), (C.c_int32 * c.t)(*range(c.t))
    in_frame, out_frame = c.h * c.w * c.cin, o.ho * o.wo * c.cout

    def call(x_off=0, in_stride=in_frame, y_off=0, out_stride=out_frame, res_off=0):
        d = _hip.Conv3dDesc(x.data_ptr() + x_off, in_stride, ins, c.h, c.w, c.cin, 0, w.data_ptr(), None, c.kt, c.ks, y.data_ptr() + y_off,
                            out_stride, outs, c.cout, c.t, res.data_ptr() + res_off, zero.data_ptr(), 0)
        _hip.check(_hip.load().ifx_conv3d_cl(C.byref(d), torch.cuda.current_stream().cuda_stream), "ifx_conv3d_cl")

    for kwargs, text in ((dict(x_off=8), "x and w must be 16-byte aligned"), (dict(in_stride=in_frame + 4), "in_frame_stride"),
                         (dict(y_off=8), "y and residual must be 16-byte aligned"), (dict(res_off=8), "y and residual must be 16-byte aligned"),
                         (dict(out_stride=out_frame + 4), "out_frame_stride")):
        with pytest.raises(_hip.HipKernelError, match=text):
            call(**kwargs)
    torch.cuda.synchronize()
    assert float((y.float() - 7.0).abs().max()) == 0.0, "a refused call wrote its output"


# ---- F: ifx_rmsnorm_cl ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c", K.NORM_CHANNELS)
def test_rmsnorm_cl_every_instantiation(ops, c, silu):
    """Three geometries per channel count (conv_cases.norm_geometries), one all-zero pixel in each (the one-pixel frame is run with a
    data pixel as well: see conv_cases.build_norm); slots that are not named keep their sentinel; where channels % 32 == 0 the planar output is to_planar of the plain one, bit for bit."""
    g_, cpl = K.norm_row(c)
    for geo, zero_pixel in ((0, False), (0, True), (1, True), (2, True)):
        o = K.build_norm(c, geo, K.SEED, zero_pixel)
        x, gamma = o.x.cuda(), o.gamma.cuda()
        y = torch.full((o.n_slots, 1, o.pixels, c), 7.0, dtype=BF, device="cuda")
        ops.rmsnorm_cl(x, gamma, y, o.out_slots, silu=silu)
        got = torch.stack([y[s] for s in o.out_slots]).cpu()
        ref = o.ref_silu if silu else o.ref
        if geo == 0 and zero_pixel:          # the one-pixel frame whose pixel is the zero pixel: the reference is all zeros, nothing but zeros will do
            assert float(ref.abs().max()) == 0.0 and float(got.abs().max()) == 0.0 and not torch.isnan(got.float()).any()
        else:
            judge("F", f"rmsnorm_cl<{g_}, {cpl}> c{c} silu{int(silu)} {o.frames}x{o.pixels}", got, ref, **K.NORM_BARS)
        if zero_pixel:
            assert float(got[o.zero_at].abs().max()) == 0.0
        unnamed = [s for s in range(o.n_slots) if s not in o.out_slots]
        assert len(unnamed) >= 2 and float((y[unnamed].float() - 7.0).abs().max()) == 0.0, "a slot that was not named was written"
        if c % 32 == 0:
            yp = torch.full((o.n_slots, c // 32, 1, o.pixels, 32), 7.0, dtype=BF, device="cuda")
            ops.rmsnorm_cl(x, gamma, yp, o.out_slots, silu=silu)
            assert torch.equal(bits(yp), bits(ops.to_planar(y)))

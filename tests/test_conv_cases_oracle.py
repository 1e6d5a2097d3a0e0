"""CPU checks of tests/conv_cases.py, the case tables and references behind the GPU tests of ifx_conv.hip (test_hip_conv_edges.py):
the Python restatement of the launch plan agrees with the recorded launches line by line; the tables reach every kernel instantiation
the library builds; the references are tight enough for the 2 % mismatch cap to bite; and the bars of the GPU tests REJECT a result with
one planted error — a dropped tap, a replicated halo column, an off-by-one upsample index, a dropped bias tail, swapped frames, a stale
history frame — on these very cases, so a kernel that made that error could not pass."""
import os
import re

import pytest
import torch

import conv_cases as K
from test_cabi_and_host import CONV_PLAN_RECORDED
from util import assert_bf16_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CONV_CASES = K.CONV_CASES + [K.INPLACE_PERSISTENT, K.overflow_case(256, 0), K.overflow_case(256, 1),
                                 K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, 0), K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, 1)]
CUS = (256, 304, 64)          # the three fake devices of tools/conv_plan_check.cpp


def _plan_header():
    with open(os.path.join(ROOT, "inferix_amd", "csrc", "ifx_conv_plan.h")) as f:
        return f.read()


def built_conv_rows():
    """The rows of kConvShapes, as the kernels are named."""
    table = re.search(r"kConvShapes\[\] = \{(.*?)\};", _plan_header(), re.S).group(1)
    rows = [f"conv_cl_kernel<{a}, {b}, {c}>" for a, b, c in re.findall(r"lock_step<(\d+), (\d+), (\d+)>\(\)", table)]
    rows += [f"pp::conv_pp_kernel<{a}, {b}>" for a, b in re.findall(r"persistent<(\d+), (\d+)>\(\)", table)]
    return rows


def built_norm_rows():
    table = re.search(r"kNormShapes\[\]\[2\] = \{(.*?)\};", _plan_header(), re.S).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", table)]


# ---- the plan restatement --------------------------------------------------------------------------------------------------------------
def test_plan_row_agrees_with_every_recorded_conv_launch():
    """Kernel name and all nine grids (three t_out x 256 / 304 / 64 CUs) of each of the 540 grouped lines (cin 64 throughout)."""
    pat = re.compile(r"conv cout +(\d+) ks (\d) ups (\d) kt (\d) variant (\d) +(\d+)x(\d+) *: void ifx::conv::(.+?) \* 512 \d+ grids (.*)")
    n = 0
    for line in CONV_PLAN_RECORDED.splitlines():
        m = pat.fullmatch(line)
        if m is None:
            assert not line.startswith("conv cout ") or " variant " not in line, line
            continue
        n += 1
        cout, ks, ups, kt, variant, hs, ws = (int(v) for v in m.groups()[:7])
        row = K.plan_row(kt, ks, ups, cout, variant)
        assert row == m.group(8), line
        for t_out, grids in re.findall(r"t(\d+) (\d+/\d+/\d+)", m.group(9)):
            total = K.plan_tiles(hs << ups, ws << ups, cout, int(t_out))[3]
            assert [K.plan_grid(row, total, cus) for cus in CUS] == [int(v) for v in grids.split("/")], (line, t_out)
    assert n == 15 * 3 * 2 * 2 * 3


def test_norm_row_agrees_with_every_recorded_norm_launch():
    pat = re.compile(r"norm channels +(\d+): void ifx::conv::rmsnorm_cl_kernel<(\d+), (\d+)> \* 256 0 grids (\d+)/(\d+)/(\d+)")
    seen = []
    for line in CONV_PLAN_RECORDED.splitlines():
        m = pat.fullmatch(line)
        if m is None:
            continue
        ch, g, cpl, *blocks = (int(v) for v in m.groups())
        seen.append(ch)
        assert K.norm_row(ch) == (g, cpl), line
        assert [K.norm_blocks(ch, px) for px in (1, 4095, 3 * 60 * 104)] == blocks, line
    assert seen == list(range(8, 513, 8))


def test_conv_table_reaches_every_instantiation():
    """All 14 rows of kConvShapes; the 96-channel 3 x 3 tiles once on the persistent kernel (conv_variant 0) and once on the lock-step
    kernel (conv_variant 1)."""
    built = built_conv_rows()
    assert len(built) == 14 and len(set(built)) == 14
    reached = {}
    for c in K.CONV_CASES:
        for v in c.variants:
            reached.setdefault(K.plan_row(c.kt, c.ks, c.ups, c.cout, v), []).append((c.name, v))
    assert set(reached) == set(built), (sorted(set(built) - set(reached)), sorted(set(reached) - set(built)))
    for ups in (0, 1):
        assert all(v == 0 for _, v in reached[f"pp::conv_pp_kernel<96, {ups}>"])
        assert all(v == 1 for _, v in reached[f"conv_cl_kernel<96, {ups}, 3>"])
    for c in K.CONV_CASES:
        if c.variants == (0,):          # the plan must not look at conv_variant where a case does not set it
            assert K.plan_row(c.kt, c.ks, c.ups, c.cout, 0) == K.plan_row(c.kt, c.ks, c.ups, c.cout, 1), c.name


def test_conv_cases_are_what_their_rows_are_for():
    """The tails each row of the table names: channel counts, ragged tiles, the frame limit, the shortest K loops."""
    C = K.CASE
    assert {c.cout % 8 for c in K.CONV_CASES} >= {0, 1, 2, 3, 4}
    assert C["cl128x1-cout260"].cout == 2 * 128 + 4 and K.plan_tiles(8, 64, 260, 1) == (1, 1, 3, 3)
    assert K.channel_tile(36) == 64 and K.channel_tile(200) == 128 and 200 % 128 != 0
    for c in K.CONV_CASES:
        assert c.t + c.kt - 1 <= K.MAXF and c.cin % 32 == 0
    assert sum(c.t + c.kt - 1 == K.MAXF for c in K.CONV_CASES) >= 4
    # K loop of the lock-step kernel: totalG = kt * (cin / 32) * (3 for a 3 x 3 kernel, 1 for 1 x 1) groups
    total_g = lambda c: c.kt * (c.cin // 32) * (3 if c.ks == 3 else 1)
    assert total_g(C["cl32x1-cout1"]) == 1 and total_g(C["cl32x3-cout2"]) == 3 and total_g(C["cl64x3-cout36"]) == 3
    # zero frames: with 1 x 1 taps, in the planar layout of the persistent kernel, and in front of a 3 x 3 lock-step launch
    assert C["cl32x1-cout20-maxf"].zero == (0, 1) and C["pp96-zero-planar"].zero_planar == (0,) and C["cl32x3-cout12-maxf"].zero == (0,)
    assert len(K.INPLACE_CASES) == 6 and all(c.res for c in K.INPLACE_CASES)
    assert K.plan_tiles(17, 130, 96, 3)[3] == 27 and K.plan_row(3, 3, 0, 96, 0).startswith("pp::")


def test_overflow_case_gives_some_workgroup_a_second_tile():
    """On 256 CUs the rule (smallest multiple of 64 plus 6 columns with more tiles than workgroups, no multiple of the grid) gives
    24 x 326: 3 x 6 x 16 = 288 tiles on 256 workgroups; the named 24 x 390 has 3 x 7 x 16 = 336.  On any CU count, more tiles than the grid."""
    c = K.overflow_case(256, 0)
    assert (c.h, c.w, c.t, c.cin, c.cout) == (24, 326, 16, 32, 96) and K.plan_tiles(24, 326, 96, 16) == (6, 3, 1, 288)
    u = K.overflow_case(256, 1)
    assert (u.h, u.w) == (12, 163)
    n = K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, 0)
    assert (n.h, n.w) == (24, 390) and K.plan_tiles(24, 390, 96, 16) == (7, 3, 1, 336) and K.plan_grid("pp::conv_pp_kernel<96, 0>", 336, 256) == 256
    assert (K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, 1).h, K.overflow_case_of_width(K.OVERFLOW_NAMED_WIDTH, 1).w) == (12, 195)
    for cus in (64, 104, 256, 304):
        for ups in (0, 1):
            c = K.overflow_case(cus, ups)
            row = K.plan_row(c.kt, c.ks, c.ups, c.cout, 0)
            total = K.plan_tiles(c.h << ups, c.w << ups, c.cout, c.t)[3]
            grid = K.plan_grid(row, total, cus)
            assert row == f"pp::conv_pp_kernel<96, {ups}>" and grid == 8 * (cus // 8) and total > grid and total % grid != 0
            assert (c.w << ups) % 64 == 6 and (c.h << ups) == 24


def test_norm_table_reaches_every_reachable_instantiation():
    """Every (G, CPL) some channel count in [8, 512] selects is named by a case; <32, 3> and <64, 3> are built but would need 768 and
    1536 channels, which ifx_rmsnorm_cl refuses (channels <= 512): unreachable, and they stay in the library as they are."""
    built = built_norm_rows()
    assert len(built) == 14
    reachable = {K.norm_row(ch) for ch in range(8, 513, 8)}
    assert set(built) - reachable == {(32, 3), (64, 3)} and reachable <= set(built)
    assert K.norm_row(768) == (32, 3) and K.norm_row(1536) == (64, 3)
    assert min(ch for ch in range(8, 4096, 8) if K.norm_row(ch) == (32, 3)) == 768
    assert min(ch for ch in range(8, 4096, 8) if K.norm_row(ch) == (64, 3)) == 1536
    table = {K.norm_row(ch) for ch in K.NORM_CHANNELS} | {K.norm_row(ch) for ch, _ in K.NORM_DECODER_CASES}
    assert table == reachable, sorted(reachable - table)
    # the rows the decoder's own widths never reach, and lane groups with masked lanes (chunks < G * CPL)
    assert {K.norm_row(ch) for ch in K.NORM_CHANNELS} >= {(1, 1), (2, 1), (8, 1), (32, 1), (64, 1), (1, 3), (2, 3)}
    for ch in (40, 72, 200, 264):
        g, cpl = K.norm_row(ch)
        assert ch in K.NORM_CHANNELS and ch // 8 < g * cpl


@pytest.mark.parametrize("ch", K.NORM_CHANNELS + tuple(sorted({c for c, _ in K.NORM_DECODER_CASES})))
def test_norm_oracle_gives_zeros_for_the_zero_pixel(ch):
    for geo in range(3):
        o = K.build_norm(ch, geo)
        assert float(o.x[o.zero_at].abs().max()) == 0.0
        for ref in (o.ref, o.ref_silu):
            assert ref.dtype == torch.bfloat16 and torch.isfinite(ref.float()).all()
            assert float(ref[o.zero_at].abs().max()) == 0.0
        frames, pixels, n_slots = K.norm_geometries(ch)[geo]
        assert frames <= K.MAXF and len(set(o.out_slots)) == frames and n_slots >= frames + 2
        # a relative bar needs a reference that is not all zeros: every geometry but the single zero pixel, which has its data twin
        assert (float(o.ref.abs().max()) > 0.0) == (geo != 0)
    twin = K.build_norm(ch, 0, K.SEED, False)
    assert twin.zero_at is None and float(twin.ref.abs().max()) > 0.0 and float(twin.ref_silu.abs().max()) > 0.0
    assert K.norm_geometries(ch)[2][1] == K.norm_pixels_per_block(ch) + 1


# ---- the references: tight, and the bars reject planted errors ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CONV_CASES, ids=lambda c: c.name)
def test_reference_is_tight_and_the_unmutated_evaluation_passes(case):
    """The 2 % mismatch cap of the GPU bars is a condition on the inputs: with 1024 elements or more, and an fp32 reference that differs
    from the fp64 evaluation in at most 0.2 % of them, a kernel has a tenth of the cap for the reference's own rounding and the rest for
    its own.  The fp64 evaluation rounded to bf16 passes the GPU bars."""
    for planar in (False, True) if case.zero_planar else (False,):
        o = K.build(case, K.SEED, planar)
        assert o.ref.numel() >= 1024 and tuple(o.ref.shape) == (case.t, o.ho, o.wo, case.cout)
        exact = K.conv_taps(o)
        frac = float((exact.view(torch.int16) != o.ref.view(torch.int16)).double().mean())
        print(f"CONVREF|{case.name}|planar{int(planar)}|fp32 vs fp64 differ {frac:.5f}")
        assert frac <= 0.002, (case.name, frac)
        assert_bf16_parity(exact, o.ref, what=case.name, **K.conv_bars(case))


def test_no_case_is_larger_than_the_largest_named():
    """24 x 390 x 96 channels x 16 frames (the overflow case) bounds every conv case; the rest are a fraction of it."""
    cap = 24 * 390 * 96 * 16
    for c in ALL_CONV_CASES:
        assert c.t * (c.h << c.ups) * (c.w << c.ups) * c.cout <= cap, c.name
    assert sum(c.t * (c.h << c.ups) * (c.w << c.ups) * c.cout for c in K.CONV_CASES) < cap // 8


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_bars_reject_the_planted_error(mutation):
    """Every case the mutation applies to, at the bars the GPU test applies to that case; and each (ks, ups) pair of the kernels has at
    least one such case wherever the mutation can exist for it (no halo with 1 x 1 taps, no upsample index without upsampling)."""
    pairs = set()
    for case in K.CONV_CASES + [K.INPLACE_PERSISTENT]:
        for planar in (False, True) if case.zero_planar else (False,):
            if not K.mutation_applies(mutation, case, planar):
                continue
            o = K.build(case, K.SEED, planar)
            wrong = K.conv_taps(o, mutation=mutation)
            with pytest.raises(AssertionError):
                assert_bf16_parity(wrong, o.ref, what=f"{case.name} {mutation}", **K.conv_bars(case))
            pairs.add((case.ks, case.ups))
    want = {"tap": {(1, 0), (3, 0), (3, 1)}, "halo": {(3, 0), (3, 1)}, "ups_index": {(3, 1)}, "bias_tail": {(1, 0), (3, 0), (3, 1)},
            "swap": {(1, 0), (3, 0), (3, 1)}, "zero_frame": {(1, 0), (3, 0)}}[mutation]      # (no decoder layer upsamples behind zero frames: kt = 1)
    assert pairs >= want, (mutation, sorted(want - pairs))

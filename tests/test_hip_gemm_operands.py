"""GPU tests of the GEMM family's OPERAND forms (ifx_gemm.hip, ifx_gemm_glds.hip, ifx_gemm_w4.hip, ifx_gemm_pp.hip, the 8-bit kernels of
ifx_quant.hip): what the other GEMM tests never hand over — row strides wider than the row, outputs that are column windows of a larger
buffer, the residual updated in place, weight row slices, N / ldy / ld_res % 8 == 4 — and the 8-bit LDS-DMA tiles against the oracle.

A FRAMED launch places every operand as a window of a larger buffer filled with sentinels:
    x        [M+8, K+72]  columns [8, 8+K)            ldx    = K+72   finite random values around it
    y        [M+8, N+40]  columns [16, 16+N), rows < M  ldy    = N+40   7.0 around it
    residual [M+8, N+24]  columns [8, 8+N)            ld_res = N+24   finite random values around it
    bias = b_big[8:8+N], w = w_big[16:16+N] (a row slice of a taller matrix), mod dense.  Every window base is 16-byte aligned.
Strides do not change a summation order: the window of a framed launch is BIT-identical to the dense launch of the same tile on the
same values, every sentinel of the output buffer is still there afterwards, and so is it when the window is residual and output at
once.  The chain of bit-equalities is anchored once per tile to torch.nn.functional.linear / the CPU oracle."""
import functools
from types import SimpleNamespace

import pytest
import torch

import quant_oracle as Q
import wan_oracle as O
from util import assert_bf16_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 7.0
BIAS, GELU_TANH, RESIDUAL, GATE_RES, GELU_ERF = 0, 1, 2, 3, 4        # IFX_EPI_* (include/inferix_hip.h)
EPILOGUES = (BIAS, GELU_TANH, GELU_ERF, RESIDUAL, GATE_RES)
EPI_NAME = {BIAS: "bias", GELU_TANH: "gelu_tanh", GELU_ERF: "gelu_erf", RESIDUAL: "residual", GATE_RES: "gate+residual"}
GATE_SLOT = 2


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def gpu(t):
    return t.cuda()


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def y_frame(M, N, width=40, col0=16):
    """(buffer [M+8, N+width] of sentinels, its window [M, N] from column col0)"""
    buf = torch.full((M + 8, N + width), SENTINEL, dtype=BF, device="cuda")
    return buf, buf[:M, col0:col0 + N]


def frame_intact(buf, M, N, col0=16):
    """every element of `buf` outside rows [0, M) x columns [col0, col0+N) still holds the sentinel"""
    chk = buf.clone()
    chk[:M, col0:col0 + N] = SENTINEL
    return bool((chk == SENTINEL).all())


def epi_kw(c, epi, res):
    kw = dict(epilogue=epi)
    if epi in (RESIDUAL, GATE_RES):
        kw["residual"] = res
    if epi == GATE_RES:
        kw.update(mod=c.mod, gate_slot=GATE_SLOT, rows_per_group=c.rpg)
    return kw


@functools.lru_cache(maxsize=None)
def bf16_case(M, N, K):
    """One seeded set of operands on the GPU, framed (`*_win`: views into sentinel-filled buffers) and dense (copies of the same
    values), and the host copies the CPU references are made of.  Shared by every test of the shape; nothing writes to it."""
    g = torch.Generator().manual_seed(M + N + K)
    c = SimpleNamespace(M=M, N=N, K=K, rpg=(M + 1) // 2)             # two gate groups: 167 rows each at M = 333
    x_big, w_big = rnd(g, M + 8, K + 72), rnd(g, N + 32, K, scale=K ** -0.5)
    b_big, res_big = rnd(g, N + 16, scale=0.1), rnd(g, M + 8, N + 24)
    c.h = SimpleNamespace(x=x_big[:M, 8:8 + K].contiguous(), w=w_big[16:16 + N].contiguous(), b=b_big[8:8 + N].contiguous(),
                          res=res_big[:M, 8:8 + N].contiguous(), mod=rnd(g, 2, 6, N, scale=0.5))
    c.x_win, c.w_win, c.b_win = gpu(x_big)[:M, 8:8 + K], gpu(w_big)[16:16 + N], gpu(b_big)[8:8 + N]
    c.res_win = gpu(res_big)[:M, 8:8 + N]
    c.x, c.w, c.b, c.res, c.mod = gpu(c.h.x), gpu(c.h.w), gpu(c.h.b), gpu(c.h.res), gpu(c.h.mod)
    assert c.x_win.stride(0) == K + 72 and c.res_win.stride(0) == N + 24
    assert all(t.data_ptr() % 16 == 0 for t in (c.x_win, c.w_win, c.b_win, c.res_win))
    return c


@functools.lru_cache(maxsize=None)
def bf16_refs(M, N, K):
    """CPU references of the five epilogues, as test_gemm_every_tile_variant forms them"""
    c = bf16_case(M, N, K)
    h = c.h
    y = torch.nn.functional.linear(h.x, h.w, h.b)
    gate = torch.repeat_interleave(h.mod[:, GATE_SLOT], c.rpg, dim=0)[:M]
    return {BIAS: y, GELU_TANH: torch.nn.functional.gelu(y, approximate="tanh"), GELU_ERF: torch.nn.functional.gelu(y),
            RESIDUAL: h.res + y, GATE_RES: h.res + (y * gate).to(BF)}


def assert_epilogue_parity(got, ref, epi, what):
    """the bars of test_gemm_every_tile_variant, per epilogue (the erf GELU is the same instantiation as the tanh one)"""
    if epi == BIAS:
        assert_bf16_parity(got, ref, what=what)
    else:
        assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, what=what)


def dense_linear(ops, c, epi):
    return ops.linear(c.x, c.w, c.b, **epi_kw(c, epi, c.res))


def check_framed(ops, c, epi, dense, what, *, y_width=40, y_col=16, res_win=None):
    """the framed launch, and for the residual epilogues the in-place one, against `dense` bit for bit; frames untouched.  A caller's
    own residual window has no part in the in-place launch (the residual is the output window there), which is left out then."""
    M, N = c.M, c.N
    in_place = res_win is None
    res_win = c.res_win if res_win is None else res_win
    buf, win = y_frame(M, N, y_width, y_col)
    got = ops.linear(c.x_win, c.w_win, c.b_win, out=win, **epi_kw(c, epi, res_win))
    assert got.data_ptr() == win.data_ptr()
    assert torch.equal(win, dense), f"{what}: the framed launch differs from the dense one"
    assert frame_intact(buf, M, N, y_col), f"{what}: a store outside the output window"
    if epi in (RESIDUAL, GATE_RES) and in_place:
        buf, win = y_frame(M, N, y_width, y_col)
        win.copy_(c.res)
        ops.linear(c.x_win, c.w_win, c.b_win, out=win, **epi_kw(c, epi, win))
        assert torch.equal(win, dense), f"{what}: the in-place launch (out = residual) differs from the out-of-place one"
        assert frame_intact(buf, M, N, y_col), f"{what}: in place, a store outside the output window"


# ---- A: the framed launch, every forced bf16 tile ----------------------------------------------------------------------------------
A_VARIANTS = [*range(1, 20), *range(21, 26)]                         # what test_gemm_every_tile_variant forces (20, 26-29: lab / large)


@pytest.mark.parametrize("variant", A_VARIANTS)
def test_gemm_bf16_framed_and_in_place_every_forced_tile(ops, variant):
    """333 rows end inside 64-, 128-, 192- and 256-row tiles, 704 channels inside 128-, 192- and 256-wide ones (and are a multiple of 64,
    which the ping-pong tiles ask for); K / 64 = 4 serves the in-workgroup K splits of 12-14; 712 channels: N % 64 == 8."""
    for M, N, K in ((333, 704, 256), (333, 712, 256)):
        if N % 64 != 0 and variant >= 22:
            continue                                                 # refused: test_gemm_bf16_ping_pong_tiles_refuse_n_712_without_a_store
        c = bf16_case(M, N, K)
        with ops.option_scope("gemm_variant", variant):
            for epi in EPILOGUES:
                what = f"variant {variant} {M}x{N}x{K} {EPI_NAME[epi]}"
                dense = dense_linear(ops, c, epi)
                if epi == BIAS:
                    assert_bf16_parity(dense, bf16_refs(M, N, K)[BIAS], what=what)        # the bar of test_gemm_bias
                check_framed(ops, c, epi, dense, what)


@pytest.mark.parametrize("variant", [22, 23, 24, 25])
def test_gemm_bf16_ping_pong_tiles_refuse_n_712_without_a_store(ops, variant):
    from inferix_amd import _hip
    c = bf16_case(333, 712, 256)
    buf, win = y_frame(c.M, c.N)
    with ops.option_scope("gemm_variant", variant):
        with pytest.raises(_hip.HipKernelError, match="multiples of 64"):
            ops.linear(c.x_win, c.w_win, c.b_win, out=win)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused launch wrote to its output"


@pytest.mark.parametrize("variant", [22, 23])
def test_gemm_bf16_split_k_in_place_residual(ops, variant):
    """K = 4096 at N = 704: gemm_pp_split holds, so the forced 256- and 192-token tiles run two workgroups per tile through the
    workspace ifx_gemm_workspace_bytes asks for and hip_ops.linear hands over.  That the split ran is seen in the workspace: its
    partial-sum area, zeroed before the launch, holds the second workgroups' fp32 tile images afterwards.  Framed + in place, gate
    epilogue: the dense launch's bits, twice, flags left zero."""
    from inferix_amd import _hip
    M, N, K = 333, 704, 4096
    c = bf16_case(M, N, K)
    ops.set_option("gemm_small_split", 0)
    with ops.option_scope("gemm_variant", variant):
        assert int(_hip.load().ifx_gemm_workspace_bytes(M, N, K)) > 4096, "the forced tile must ask for the split-K workspace"
        dense = dense_linear(ops, c, GATE_RES)
        for ws in ops._GEMM_WS.values():
            ws[4096:].zero_()
        assert torch.equal(dense, dense_linear(ops, c, GATE_RES)), "split-K is not deterministic"
        assert any(bool(ws[4096:].any()) for ws in ops._GEMM_WS.values()), "no partial sums in the workspace: K was not split"
        for _ in range(2):
            check_framed(ops, c, GATE_RES, dense, f"variant {variant} split-K")
    torch.cuda.synchronize()
    for ws in ops._GEMM_WS.values():
        assert int(ws[:4096].view(torch.int32).abs().sum().item()) == 0, "per-tile flags must be left zero"
    assert_epilogue_parity(dense, bf16_refs(M, N, K)[GATE_RES], GATE_RES, f"variant {variant} split-K vs CPU")


# ---- B: the narrow fallbacks ---------------------------------------------------------------------------------------------------------
B_FORCED = (0, 3, 5, 19, 22)          # auto and forced LDS-DMA / four-wave / ping-pong tiles: all must end in the register-staged kernel


@pytest.mark.parametrize("M,N,K", [(77, 68, 64), (300, 132, 256), (333, 644, 256)])
def test_gemm_bf16_narrow_n_runs_the_register_kernel(ops, M, N, K):
    """N % 8 == 4: no 16-byte epilogue vector fits a row, so every choice has to fall to the register-staged 128x128 kernel (8-byte
    vectors) — the same bits as forced variant 1, never dropped columns — dense and framed (ldy = N + 40 and ld_res = N + 24 are
    % 8 == 4 as well here)."""
    c, refs = bf16_case(M, N, K), bf16_refs(M, N, K)
    with ops.option_scope("gemm_variant", 1):
        base = {epi: dense_linear(ops, c, epi) for epi in EPILOGUES}
    for epi in EPILOGUES:
        assert_epilogue_parity(base[epi], refs[epi], epi, f"variant 1 {M}x{N}x{K} {EPI_NAME[epi]}")
    for variant in B_FORCED:
        with ops.option_scope("gemm_variant", variant):
            for epi in EPILOGUES:
                what = f"variant {variant} {M}x{N}x{K} {EPI_NAME[epi]}"
                assert torch.equal(dense_linear(ops, c, epi), base[epi]), f"{what}: not the register-staged kernel's bits"
                check_framed(ops, c, epi, base[epi], what)


def test_gemm_bf16_narrow_strides_and_8_byte_windows_run_the_register_kernel(ops):
    """N = 704 would take the wide tiles; a row stride % 8 == 4 or a window base that is only 8-byte aligned must not:
      ldy = N + 44, y window at column 4 (also in place: ld_res = ldy);  ld_res = N + 28, residual window at column 4;
      ldy = N + 40 with the y window at column 4 — the strides fit, the BASE is 8-byte aligned: the launcher looks at the pointers too
      (also in place: residual and output on that base).
    x, W and bias stay 16-byte aligned.  Every access of the register-staged kernel is naturally aligned on these operands
    (16-byte loads of x / W rows, 8-byte bias / residual / gate / y vectors at columns % 4 == 0)."""
    M, N, K = 333, 704, 256
    c, refs = bf16_case(M, N, K), bf16_refs(M, N, K)
    g = torch.Generator().manual_seed(28)
    res_big = gpu(rnd(g, M + 8, N + 28))
    res_narrow = res_big[:M, 4:4 + N]
    res_narrow.copy_(c.res)
    assert res_narrow.data_ptr() % 16 == 8 and res_narrow.stride(0) % 8 == 4
    with ops.option_scope("gemm_variant", 1):
        base = {epi: dense_linear(ops, c, epi) for epi in EPILOGUES}
    for epi in EPILOGUES:
        assert_epilogue_parity(base[epi], refs[epi], epi, f"variant 1 {M}x{N}x{K} {EPI_NAME[epi]}")
    for variant in B_FORCED:
        with ops.option_scope("gemm_variant", variant):
            for epi in EPILOGUES:
                what = f"variant {variant} {EPI_NAME[epi]}"
                check_framed(ops, c, epi, base[epi], what + ", ldy = N + 44", y_width=44, y_col=4)
                check_framed(ops, c, epi, base[epi], what + ", 8-byte aligned y", y_width=40, y_col=4)
                if epi in (RESIDUAL, GATE_RES):
                    check_framed(ops, c, epi, base[epi], what + ", ld_res = N + 28", res_win=res_narrow)


# ---- C: the 8-bit kernels ------------------------------------------------------------------------------------------------------------
def q8_rows(M):
    """the rows compared with the CPU oracle where all of them would take it too long: first 64, 64 around the middle, last 64"""
    return torch.cat([torch.arange(0, 64), torch.arange(M // 2 - 32, M // 2 + 32), torch.arange(M - 64, M)])


@functools.lru_cache(maxsize=None)
def q8_case(M, N, K, fmt):
    """As bf16_case for the 8-bit linears: x quantised per token and W per channel on the GPU (both pinned to the oracle bit for bit by
    tests/test_hip_quant.py).  Frames: xq [M+8, K+80] bytes, window from byte column 16; y, residual and bias as in bf16_case; wq and
    w_scale dense."""
    from inferix_amd import hip_ops as ops
    from inferix_amd.quant import QConfig, quantize_weight
    g = torch.Generator().manual_seed(M + N + K + fmt)
    c = SimpleNamespace(M=M, N=N, K=K, fmt=fmt, rpg=M // 2 + 1)
    b_big, res_big = rnd(g, N + 16, scale=0.1), rnd(g, M + 8, N + 24)
    c.h = SimpleNamespace(x=rnd(g, M, K), w=rnd(g, N, K, scale=K ** -0.5), b=b_big[8:8 + N].contiguous(),
                          res=res_big[:M, 8:8 + N].contiguous(), mod=rnd(g, 2, 6, N, scale=0.5))
    c.wq, c.sw = quantize_weight(gpu(c.h.w), QConfig(fmt, "t"))
    c.xq, c.sx = ops.quant_per_token(gpu(c.h.x), fmt)
    xq_big = torch.randint(0, 256, (M + 8, K + 80), generator=g, dtype=torch.uint8).cuda()
    c.xq_win = xq_big[:M, 16:16 + K]
    c.xq_win.copy_(c.xq)
    c.b_win, c.res_win = gpu(b_big)[8:8 + N], gpu(res_big)[:M, 8:8 + N]
    c.b, c.res, c.mod = gpu(c.h.b), gpu(c.h.res), gpu(c.h.mod)
    assert c.xq_win.stride(0) == K + 80 and all(t.data_ptr() % 16 == 0 for t in (c.xq_win, c.b_win, c.res_win, c.sw, c.wq))
    return c


def q8_linear(ops, c, epi, *, framed=False, bias=True, res=None, out=None):
    xq, b = (c.xq_win, c.b_win) if framed else (c.xq, c.b)
    res = res if res is not None else (c.res_win if framed else c.res)
    return ops.linear_q8(xq, c.sx, c.wq, c.sw, b if bias else None, c.fmt, out=out, **epi_kw(c, epi, res))


def q8_gate_ref(res, y, mod, rpg, rows):
    """wan_oracle.gated_residual group by group (the groups of `rows_per_group` rows need not divide the row count)"""
    out = torch.empty_like(y)
    grp = rows // rpg
    for gi in grp.unique().tolist():
        sel = grp == gi
        out[sel] = O.gated_residual(res[None, sel], y[None, sel], mod[gi, GATE_SLOT][None, None, None, :], 1)[0]
    return out


@functools.lru_cache(maxsize=None)
def q8_refs(M, N, K, fmt):
    """(rows, oracle results on those rows): all rows where quant_oracle.linear_q8 takes about a second, else q8_rows(M)"""
    c = q8_case(M, N, K, fmt)
    h = c.h
    rows = torch.arange(M) if M * N * K <= 2300 * 3208 * 256 else q8_rows(M)
    y = Q.linear_q8(h.x[rows], h.w, h.b, fmt)
    return rows, {"plain": Q.linear_q8(h.x[rows], h.w, None, fmt), BIAS: y,
                  GELU_TANH: torch.nn.functional.gelu(y, approximate="tanh"), RESIDUAL: h.res[rows] + y,
                  GATE_RES: q8_gate_ref(h.res[rows], y, h.mod, c.rpg, rows)}


@pytest.mark.parametrize("fmt", [Q.FP8, Q.INT8])
@pytest.mark.parametrize("variant", [3, 2])
@pytest.mark.parametrize("M,N,K", [(2300, 3208, 256), (4090, 8200, 256)])
def test_gemm_q8_lds_dma_tiles_vs_oracle(ops, M, N, K, variant, fmt):
    """gemm_q8_dma_kernel<256,128> (9 x 26 = 234 tiles of 256 x 128: >= 224, and fewer than 512 of 256 x 256) and <256,256> (16 x 33 = 528
    tiles), both ragged in rows and channels (N % 64 == 8: the ping-pong tile declines under auto too), in the 128-byte-row form
    (variant 3: three / two stages) and the 64-byte-row four-stage form (variant 2); every epilogue against quant_oracle.linear_q8 /
    wan_oracle.gated_residual with the bars test_gemm_q8_ping_pong_tiles_vs_oracle uses.  The 4090 x 8200 case compares the first 64
    rows, 64 rows around the middle and the last 64 (the ragged tile) over all columns; the 2300 x 3208 case every row."""
    c = q8_case(M, N, K, fmt)
    rows, refs = q8_refs(M, N, K, fmt)
    on = lambda t: t[rows.cuda()].cpu()
    what = f"q8 LDS-DMA v{variant} fmt={fmt} {M}x{N}x{K}"
    with ops.option_scope("gemm_variant", variant):
        got = {epi: on(q8_linear(ops, c, epi)) for epi in (BIAS, GELU_TANH, RESIDUAL, GATE_RES)}
        plain = on(q8_linear(ops, c, BIAS, bias=False))
    assert_bf16_parity(got[BIAS], refs[BIAS], what=what)
    assert_bf16_parity(plain, refs["plain"], what=what + " no bias")
    assert_bf16_parity(got[GELU_TANH], refs[GELU_TANH], max_ulp=4, max_mismatch_frac=0.05, rel=3e-3, floor=1.0, what=what + " gelu")
    assert_bf16_parity(got[RESIDUAL], refs[RESIDUAL], max_ulp=2, floor=1.0, what=what + " residual")
    assert_bf16_parity(got[GATE_RES], refs[GATE_RES], max_ulp=4, max_mismatch_frac=0.03, floor=1.0, what=what + " gate")


Q8_FRAMED = [(1, 333, 704, 256),           # the register-staged gemm_q8_kernel
             (3, 2300, 3208, 256),         # the 256x128 LDS-DMA tile
             (22, 1100, 704, 256), (23, 1100, 704, 256), (24, 1100, 704, 256),      # the ping-pong tiles
             (0, 333, 708, 256)]           # N % 8 == 4 under auto: the register-staged kernel


def check_q8_framed(ops, c, epi, dense, what):
    """the framed 8-bit launch, and for the residual epilogues the in-place one, against `dense` bit for bit; frames untouched"""
    M, N = c.M, c.N
    buf, win = y_frame(M, N)
    q8_linear(ops, c, epi, framed=True, out=win)
    assert torch.equal(win, dense), f"{what}: the framed launch differs from the dense one"
    assert frame_intact(buf, M, N), f"{what}: a store outside the output window"
    if epi in (RESIDUAL, GATE_RES):
        buf, win = y_frame(M, N)
        win.copy_(c.res)
        q8_linear(ops, c, epi, framed=True, res=win, out=win)
        assert torch.equal(win, dense), f"{what}: the in-place launch (out = residual) differs from the out-of-place one"
        assert frame_intact(buf, M, N), f"{what}: in place, a store outside the output window"


@pytest.mark.parametrize("fmt", [Q.FP8, Q.INT8])
@pytest.mark.parametrize("variant,M,N,K", Q8_FRAMED)
def test_gemm_q8_framed_and_in_place(ops, variant, M, N, K, fmt):
    """The framed and in-place checks of the bf16 tiles on four 8-bit kernel families: bit-equal to the dense launch of the same tile,
    frame untouched.  xq rows are 80 bytes apart from dense (ldx = K + 80, window at byte 16)."""
    c = q8_case(M, N, K, fmt)
    with ops.option_scope("gemm_variant", variant):
        for epi in (BIAS, GELU_TANH, RESIDUAL, GATE_RES):
            check_q8_framed(ops, c, epi, q8_linear(ops, c, epi), f"q8 v{variant} fmt={fmt} {M}x{N}x{K} {EPI_NAME[epi]}")


@pytest.mark.parametrize("fmt", [Q.FP8, Q.INT8])
def test_gemm_q8_narrow_n_runs_the_register_kernel(ops, fmt):
    """2300 x 3212: with N % 8 == 0 the auto choice and forced variants 2 / 3 would run the 256x128 LDS-DMA tile here (9 x 26 tiles),
    22 the ping-pong tile; N % 8 == 4 must send all of them to the register-staged gemm_q8_kernel — forced variant 1's bits, dense and
    framed (333 x 708 in the test above runs that kernel whatever N is)."""
    M, N, K = 2300, 3212, 256
    c = q8_case(M, N, K, fmt)
    epis = (BIAS, GELU_TANH, RESIDUAL, GATE_RES)
    with ops.option_scope("gemm_variant", 1):
        base = {epi: q8_linear(ops, c, epi) for epi in epis}
    rows = q8_rows(M)
    y = Q.linear_q8(c.h.x[rows], c.h.w, c.h.b, fmt)
    assert_bf16_parity(base[BIAS][rows.cuda()], y, what=f"q8 variant 1 fmt={fmt} {M}x{N}x{K}")
    assert_bf16_parity(base[GATE_RES][rows.cuda()], q8_gate_ref(c.h.res[rows], y, c.h.mod, c.rpg, rows), max_ulp=4, max_mismatch_frac=0.03,
                       floor=1.0, what=f"q8 variant 1 fmt={fmt} {M}x{N}x{K} gate")
    for variant in (0, 2, 3, 22):
        with ops.option_scope("gemm_variant", variant):
            for epi in epis:
                what = f"q8 v{variant} fmt={fmt} {M}x{N}x{K} {EPI_NAME[epi]}"
                assert torch.equal(q8_linear(ops, c, epi), base[epi]), f"{what}: not the register-staged kernel's bits"
                check_q8_framed(ops, c, epi, base[epi], what)


# ---- D: the product's calls under the auto choice ------------------------------------------------------------------------------------
def test_gemm_auto_t5_in_place_residual(ops):
    """inferix_amd/t5.py: `linear(h, w, None, epilogue=RESIDUAL, residual=x, out=x)` at 512 x 4096 x 4096"""
    g = torch.Generator().manual_seed(4096)
    M, N, K = 512, 4096, 4096
    h, w, x = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, M, N))
    want = ops.linear(h, w, None, epilogue=RESIDUAL, residual=x)
    stream = x.clone()
    got = ops.linear(h, w, None, epilogue=RESIDUAL, residual=stream, out=stream)
    assert got.data_ptr() == stream.data_ptr() and torch.equal(stream, want)


def test_gemm_auto_vae_scores_into_a_column_window(ops):
    """inferix_amd/vae.py: the attention scores of the middle block, `out=s_buf[:, :hw]`, hw = 6240 in a buffer 6272 wide, K = 384"""
    g = torch.Generator().manual_seed(6240)
    hw, ch, width = 6240, 384, 6272
    q, k = gpu(rnd(g, hw, ch)), gpu(rnd(g, hw, ch, scale=ch ** -0.5))
    want = ops.linear(q, k, None)
    buf = torch.full((hw, width), SENTINEL, dtype=BF, device="cuda")
    ops.linear(q, k, None, out=buf[:, :hw])
    assert torch.equal(buf[:, :hw], want)
    assert bool((buf[:, hw:] == SENTINEL).all()), "columns [6240, 6272) were written"

"""GPU: the two kernels MAGI-24B's layer adds to the 4.5B one — `ifx_silu_and_mul` (the gated MLP's activation, bf16 and / or
the e4m3 bytes of an FP8 fc2's input) and the 12-chunk rung of the LayerNorm ladder (hidden 6144) — each against its CPU oracle."""
import pytest
import torch
import torch.nn.functional as F

import wan_oracle as O
from util import assert_bf16_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROWS = 9


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def window(t, col0, fill):
    """(buffer, view): `t` as the column window [col0, col0 + cols) of a wider device buffer filled with `fill` — NaN around an input
    (a read outside the window poisons the result), a finite sentinel around an output (a write outside it is seen).  (The pattern of
    tests/test_hip_row_kernels.py.)"""
    rows, cols = t.shape
    buf = torch.full((rows, cols + col0 + 40), fill, dtype=t.dtype, device="cuda")      # the row stride depends on col0
    view = buf[:, col0:col0 + cols]
    view.copy_(t)
    return buf, view


def margins_intact(buf, col0, cols, fill):
    return bool((buf[:, :col0] == fill).all()) and bool((buf[:, col0 + cols:] == fill).all())


def _gate_up(rows, f):
    g = torch.Generator().manual_seed(rows * 100003 + f)
    x = (2.0 * torch.randn(rows, 2 * f, generator=g)).to(BF)
    return x, F.silu(x[:, :f]) * x[:, f:]          # the oracle chain (magi_block_oracle.py:300-302): two bf16 roundings


# (1, 8): one lane; (9, 264): 33 chunks per row, rows straddle the lanes of a wave; (333, 1160): more than one block, ragged;
# (96, 16384): the 24B width, 196 608 chunks per 2048-block pass of the grid-stride loop
SHAPES = [(1, 8), (9, 264), (333, 1160), (96, 16384)]


@pytest.mark.parametrize("rows,f", SHAPES)
def test_silu_and_mul_vs_oracle_chain(ops, rows, f):
    """The bar of the project's other gated activation (tests/test_hip_t5.py): 2 ULP, at most 2 % of the elements off at all — a
    condition, not a measurement: the chain against itself is at 0, and the one-rounding form (fp32 kept between SiLU and the product)
    differs from it in 26-28 % of the elements."""
    x, ref = _gate_up(rows, f)
    frac, r = assert_bf16_parity(ops.silu_and_mul(x.cuda()), ref, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what=f"silu_and_mul {rows}x{f}")
    print(f"silu_and_mul {rows} x {f}: {frac:.5f} of the elements differ from the oracle chain, rel L2 {r:.2e}")


@pytest.mark.parametrize("rows,f", [(9, 264), (333, 1160)])
def test_silu_and_mul_in_column_windows(ops, rows, f):
    """x read from a column window of a wider NaN-filled buffer (ldx > 2f), y and q written into windows of sentinel-filled ones:
    the same bits as the dense launch, margins intact."""
    from inferix_amd import _hip
    x, ref = _gate_up(rows, f)
    dense = ops.silu_and_mul(x.cuda())
    xbuf, xv = window(x, 16, float("nan"))
    ybuf, yv = window(torch.zeros(rows, f, dtype=BF), 24, 7.0)
    qbuf, qv = window(torch.zeros(rows, f, dtype=torch.uint8), 16, 0x5A)
    div = (0.03 * (1 + 0.5 * torch.rand(f, generator=torch.Generator().manual_seed(f)))).cuda()
    ops.silu_and_mul(xv, out=yv, quant_divisor=div, q=qv)
    assert_bf16_parity(yv, ref, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what=f"silu_and_mul window {rows}x{f}")
    assert torch.equal(yv, dense)
    assert torch.equal(qv, ops.quant_static(dense, div, _hip.IFX_Q_FP8_E4M3, via_bf16=True))
    assert margins_intact(ybuf, 24, f, 7.0) and margins_intact(qbuf, 16, f, 0x5A)


@pytest.mark.parametrize("rows", [1, 9, 333])
@pytest.mark.parametrize("f", [264, 1160])
def test_silu_and_mul_quantised_output_is_quant_static_of_the_bf16_result(ops, rows, f):
    """q of the fused call == ifx_quant_static (e4m3, bf16 intermediate) of the bf16 result, every byte: per-channel divisor `[f]`,
    single divisor `[1]`, q alone and next to y."""
    from inferix_amd import _hip
    x, _ = _gate_up(rows, f)
    x = x.cuda()
    y = ops.silu_and_mul(x)
    g = torch.Generator().manual_seed(f + rows)
    for div in ((0.03 * (1 + 0.5 * torch.rand(f, generator=g))).cuda(), torch.full((1,), 0.05, device="cuda")):
        want = ops.quant_static(y, div, _hip.IFX_Q_FP8_E4M3, via_bf16=True)
        q = ops.silu_and_mul(x, quant_divisor=div)
        assert q.dtype == torch.uint8 and torch.equal(q, want), (rows, f, div.numel(), int((q != want).sum()))
        y2, q2 = ops.silu_and_mul(x, out=torch.empty_like(y), quant_divisor=div)
        assert torch.equal(y2, y) and torch.equal(q2, want), (rows, f, div.numel())


# ---------------------------------------------------------------------------------------------------------------------------------
def _offset_rows(g, dim):
    """The rows of tests/test_hip_row_kernels.py: 2 * randn with means -3, -2.25 .. 3 — a lane of a chunk beyond `dim` left inside
    the squared deviations adds mean^2, which these rows show."""
    return (2.0 * torch.randn(1, ROWS, dim, generator=g) + 0.75 * (torch.arange(float(ROWS)) - 4).view(1, ROWS, 1)).to(BF)


@pytest.mark.parametrize("dim", [5632, 6144])
def test_layernorm_on_the_12_chunk_rung(ops, dim):
    """5632: 11 chunks on the 12-chunk kernel (a whole idle chunk); 6144: all twelve.  Inputs of
    test_layernorm_every_rung_and_gap (tests/test_hip_row_kernels.py), every mode at 1 ULP (that test gives the modulated form 2)."""
    g = torch.Generator().manual_seed(dim)
    rpg, groups = 3, ROWS // 3
    x = _offset_rows(g, dim)
    assert_bf16_parity(ops.layernorm(x.cuda(), 1e-6), O.layer_norm(x, 1e-6), max_ulp=1, what=f"LN plain {dim}", report=True)
    w, b = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF), (0.1 * torch.randn(dim, generator=g)).to(BF)
    assert_bf16_parity(ops.layernorm(x.cuda(), 1e-6, gamma=w.cuda(), beta=b.cuda()), O.layer_norm(x, 1e-6, w, b), max_ulp=1,
                       what=f"LN affine {dim}", report=True)
    mod = (torch.randn(groups, 6, dim, generator=g) * 0.5).to(BF)
    e = mod.unsqueeze(0).chunk(6, dim=2)
    for shift_slot, scale_slot in ((0, 1), (3, 4)):
        ref = O.modulate(O.layer_norm(x, 1e-6), e[scale_slot], e[shift_slot], groups)
        got = ops.layernorm(x.cuda(), 1e-6, mod=mod.cuda(), shift_slot=shift_slot, scale_slot=scale_slot, rows_per_group=rpg)
        assert_bf16_parity(got, ref, max_ulp=1, floor=1.0, what=f"AdaLN {dim} slots {shift_slot},{scale_slot}", report=True)


@pytest.mark.parametrize("dim", [5632, 6144])
def test_layernorm_quant_static_on_the_12_chunk_rung(ops, dim):
    """ifx_layernorm_quant_static == ifx_layernorm then ifx_quant_static per divisor, every byte (plain and affine, two divisors)."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(dim + 1)
    x = _offset_rows(g, dim)[0].cuda()
    gamma = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF).cuda()
    beta = (0.1 * torch.randn(dim, generator=g)).to(BF).cuda()
    divs = (0.03 * (1 + 0.5 * torch.rand(2, dim, generator=g))).cuda().contiguous()
    for kw in (dict(gamma=gamma, beta=beta), {}):
        fused = ops.layernorm_quant_static(x, 1e-6, divs, **kw)
        ln = ops.layernorm(x, 1e-6, **kw)
        for j in range(2):
            assert torch.equal(fused[:, j], ops.quant_static(ln, divs[j], _hip.IFX_Q_FP8_E4M3, via_bf16=True)), (dim, j, bool(kw))


def test_layernorm_beyond_the_ladder_is_refused(ops):
    from inferix_amd import _hip
    for dim in (6152, 6656):
        x = torch.zeros(ROWS, dim, dtype=BF, device="cuda")
        with pytest.raises(_hip.HipKernelError, match=str(dim)):
            ops.layernorm(x, 1e-6)
        with pytest.raises(_hip.HipKernelError, match=str(dim)):
            ops.layernorm_quant_static(x, 1e-6, torch.ones(1, dim, device="cuda"))

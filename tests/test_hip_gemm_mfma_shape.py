"""The persistent ping-pong GEMM tile on v_mfma_f32_16x16x32_bf16 (bf16 operands): the six linear layers of a 480p block at 4680 rows
with the epilogues the block uses, against an fp64 device sum; run-to-run determinism of the split-K form; row invariance; the second
destination; and bit equality with the 256 x 256 tile of ifx_gemm_glds.hip (still on 32x32x16: same K order, same fp32 results)."""
import pytest
import torch

from util import assert_bf16_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
M, D, F, FS = 4680, 1536, 8960, 1560

# name, N, K, epilogue of the block (Wan attention block: q|k|v, o + gate, cross-q, cross-o + residual, FFN up + GELU, FFN down + gate)
BLOCK = [("qkv", 3 * D, D, "bias"), ("o", D, D, "gate"), ("cross_q", D, D, "bias"), ("cross_o", D, D, "res"),
         ("ffn_up", F, D, "gelu"), ("ffn_down", D, F, "gate")]


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    hip_ops.set_option("gemm_small_split", 0)
    return hip_ops


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF).cuda()


def operands(seed, N, K, rows=M):
    g = torch.Generator().manual_seed(seed)
    x, w, b = rnd(g, rows, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
    res, mod = rnd(g, rows, N), rnd(g, (rows + FS - 1) // FS, 6, N, scale=0.5)
    return x, w, b, res, mod


def epi_kwargs(epi, res, mod):
    from inferix_amd import _hip
    if epi == "gate":
        return dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=5, rows_per_group=FS)
    if epi == "res":
        return dict(epilogue=_hip.IFX_EPI_RESIDUAL, residual=res)
    if epi == "gelu":
        return dict(epilogue=_hip.IFX_EPI_GELU_TANH)
    return {}


@pytest.mark.parametrize("name,N,K,epi", BLOCK, ids=[b[0] for b in BLOCK])
def test_block_shapes_vs_fp64(ops, name, N, K, epi):
    """y = epilogue(bf16(x W^T + b)) with the sum in fp64 on the device, every row and channel: the bf16 result of the fp32 MFMA
    accumulation may flip one rounding in a few elements per thousand."""
    x, w, b, res, mod = operands(100 + [b[0] for b in BLOCK].index(name), N, K)
    acc = torch.empty(M, N, dtype=torch.float64, device="cuda")
    wd = w.double().t().contiguous()
    for r0 in range(0, M, 1170):
        acc[r0:r0 + 1170] = x[r0:r0 + 1170].double() @ wd
    y = (acc + b.double()).to(BF)
    del acc, wd
    got = ops.linear(x, w, b, **epi_kwargs(epi, res, mod))
    if epi == "bias":
        assert_bf16_parity(got, y, max_ulp=1, floor=0.05, what=f"{name} bias")
    elif epi == "gelu":
        want = torch.nn.functional.gelu(y, approximate="tanh")
        assert_bf16_parity(got, want, max_ulp=2, floor=1.0, max_mismatch_frac=0.03, what=f"{name} gelu")
    elif epi == "res":
        want = (res.float() + y.float()).to(BF)
        assert_bf16_parity(got, want, max_ulp=2, floor=1.0, what=f"{name} residual")
    else:
        gate = torch.repeat_interleave(mod[:, 5], FS, dim=0)[:M]
        want = (res.float() + (y.float() * gate.float()).to(BF).float()).to(BF)
        assert_bf16_parity(got, want, max_ulp=2, floor=1.0, what=f"{name} gate + residual")


def test_split_k_deterministic_and_rows_invariant(ops):
    """FFN down (K = 8960: split over two workgroups per tile) and q|k|v (unsplit): the same bits run to run, and a row's bits do not
    depend on the number of rows in the launch (4680 rows == the first 4680 of 9360)."""
    from inferix_amd import _hip
    for name, N, K, epi in (BLOCK[5], BLOCK[0]):
        x, w, b, res, mod = operands(11, N, K, rows=2 * M)
        assert (_hip.load().ifx_gemm_workspace_bytes(M, N, K) > 0) == (K == F)
        kw = epi_kwargs(epi, res[:M], mod)
        outs = [ops.linear(x[:M], w, b, **kw) for _ in range(4)]
        assert all(torch.equal(o, outs[0]) for o in outs), f"{name}: the result changed run to run"
        both = ops.linear(x, w, b, **epi_kwargs(epi, res, mod))
        assert torch.equal(both[:M], outs[0]), f"{name}: a row's bits changed with the number of rows in the launch"


def test_second_destination_matches_plain_launch(ops):
    x, w, b, _, _ = operands(12, 3 * D, D)
    plain = ops.linear(x, w, b)
    out = torch.full((M, 3 * D), 3.0, dtype=BF, device="cuda")
    v = torch.full((M, D), 7.0, dtype=BF, device="cuda")
    ops.linear(x, w, b, out=out, out2=v, split_col=2 * D)
    assert torch.equal(out[:, :2 * D], plain[:, :2 * D])
    assert torch.equal(v, plain[:, 2 * D:])
    assert bool((out[:, 2 * D:] == 3.0).all())


@pytest.mark.parametrize("name,N,K,epi", BLOCK, ids=[b[0] for b in BLOCK])
def test_ping_pong_equals_glds_tile_bitwise(ops, name, N, K, epi):
    """The 16x16x32 ping-pong tile gives the bits of the 32x32x16 256 x 256 tile (gemm_variant 5) on every block shape: the same K
    order, and the two MFMA shapes round the fp32 sums alike.  FFN down is compared unsplit (variant 25 = the single-pass ping-pong
    tile): the split adds two K halves, which the 256 x 256 tile does not."""
    x, w, b, res, mod = operands(13, N, K)
    kw = epi_kwargs(epi, res, mod)
    try:
        ops.set_option("gemm_variant", 25 if K == F else 0)
        pp = ops.linear(x, w, b, **kw)
        ops.set_option("gemm_variant", 5)
        ref = ops.linear(x, w, b, **kw)
    finally:
        ops.set_option("gemm_variant", 0)
    assert torch.equal(pp, ref), f"{name}: the ping-pong tile and the 256 x 256 tile differ"

"""The twelve-wave (loader-wave) form of the bf16 128-token ping-pong tile: four waves issue every LDS-DMA request of the eight compute
waves, which keep their tile, MFMA sequence, K order and epilogue.  Only who issues the requests changes, so its outputs must be the bits
of the eight-wave form (option gemm_pp_variant 1) and of the 256 x 256 tile (gemm_variant 5) on the three K = N = 1536 launches of a 480p block,
at a full and a ragged row count, run after run, and a row's bits must not depend on how many rows the launch has."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
M, D, FS = 4680, 1536, 1560

# the launches on the 128-token tile: O projection + gate + residual, cross-attention q, cross-attention o + residual
TRIO = [("o", "gate"), ("cross_q", "bias"), ("cross_o", "res")]


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    hip_ops.set_option("gemm_small_split", 0)
    return hip_ops


def operands(seed, rows):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF).cuda()

    x, w, b = rnd(rows, D), rnd(D, D, scale=D ** -0.5), rnd(D, scale=0.1)
    res, mod = rnd(rows, D), rnd((rows + FS - 1) // FS, 6, D, scale=0.5)
    return x, w, b, res, mod


def epi_kwargs(epi, res, mod):
    from inferix_amd import _hip
    if epi == "gate":
        return dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=2, rows_per_group=FS)
    if epi == "res":
        return dict(epilogue=_hip.IFX_EPI_RESIDUAL, residual=res)
    return {}


def run(ops, variant, x, w, b, kw, eight_waves=False):
    try:
        ops.set_option("gemm_variant", variant)
        ops.set_option("gemm_pp_variant", int(eight_waves))
        return ops.linear(x, w, b, **kw)
    finally:
        ops.set_option("gemm_variant", 0)
        ops.set_option("gemm_pp_variant", 0)


@pytest.mark.parametrize("rows", [M, M - 1])
@pytest.mark.parametrize("name,epi", TRIO, ids=[t[0] for t in TRIO])
def test_loader_waves_equal_eight_wave_form_and_glds_tile(ops, name, epi, rows):
    """Auto (the loader-wave form on these shapes), the forced 128-token tile (gemm_variant 24, the same form), the eight-wave form
    (gemm_pp_variant 1) and the 256 x 256 LDS-DMA tile (gemm_variant 5): one set of bits.  4679 rows: the last tile reads zero rows past M through the descriptor bound."""
    x, w, b, res, mod = operands(31 + [t[0] for t in TRIO].index(name), rows)
    kw = epi_kwargs(epi, res, mod)
    new = run(ops, 0, x, w, b, kw)
    assert torch.equal(run(ops, 24, x, w, b, kw), new), f"{name} at {rows} rows: gemm_variant 24 and auto differ"
    assert torch.equal(run(ops, 0, x, w, b, kw, eight_waves=True), new), f"{name} at {rows} rows: the loader-wave and the eight-wave form differ"
    assert torch.equal(run(ops, 5, x, w, b, kw), new), f"{name} at {rows} rows: the loader-wave form and the 256 x 256 tile differ"


@pytest.mark.parametrize("name,epi", TRIO, ids=[t[0] for t in TRIO])
def test_loader_waves_deterministic_and_rows_invariant(ops, name, epi):
    """The same bits run to run; the first 4680 rows of a 9360-row launch (two tiles per workgroup: the request stream runs across
    output tiles) equal a 4680-row launch (one tile per workgroup)."""
    x, w, b, res, mod = operands(41, 2 * M)
    kw = epi_kwargs(epi, res[:M], mod)
    outs = [ops.linear(x[:M], w, b, **kw) for _ in range(4)]
    assert all(torch.equal(o, outs[0]) for o in outs), f"{name}: the result changed run to run"
    # (auto takes the 256-token tile at 9360 rows: gemm_variant 24 keeps the 128-token tile, i.e. the loader-wave form)
    both = run(ops, 24, x, w, b, epi_kwargs(epi, res, mod))
    assert torch.equal(both[:M], outs[0]), f"{name}: a row's bits changed with the number of rows in the launch"
    assert torch.equal(both, run(ops, 24, x, w, b, epi_kwargs(epi, res, mod), eight_waves=True)), f"{name}: 9360 rows differ from the eight-wave form"

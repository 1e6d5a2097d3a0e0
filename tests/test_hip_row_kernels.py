"""GPU oracle tests of the row kernels' shared arithmetic (inferix_amd/csrc/ifx_rows.h: the register row, LayerNorm statistics, the
per-token quantiser, RoPE, the NCH width ladders).  The "fused producer == separate passes" tests compare that header with itself;
here every op meets an independent CPU oracle on every rung of its ladder, on the gap widths that run the next rung with whole
chunks beyond `dim`, on ragged tails, on row strides and page tables no model path sets, and on rows whose mean dwarfs their spread.

Which width runs which rung (NCH = number of 512-channel chunks the kernel is built for; "gap" = NCH > ceil(dim / 512)):
  ifx_layernorm / ifx_rmsnorm / append / push <1,2,3,4,6,8,10>:
      8 -> 1 (one lane), 512 -> 1, 520 -> 2 (one lane of chunk 1), 1024 -> 2, 2560 -> 6 (gap, 5 chunks), 3072 -> 6, 3584 -> 8 (gap, 7),
      4096 -> 8, 4608 -> 10 (gap, 9), 5120 -> 10; rung 3 (1536) and 4 (2048, 1160) are in tests/test_hip_kernels.py.
  ifx_quant_per_token <1,3,6,10,18,generic>:
      8, 512 -> 1; 520, 1024 -> 3 (gap, 2 chunks); 2048 -> 6 (gap, 4); 3072 -> 6; 5120 -> 10; 5632 -> 18 (gap, 11); 9216 -> 18;
      9224, 12288 -> the generic loop.
  ifx_magi_gate_norm_residual <1,2,4,6,8,12>:
      520 -> 2, 1024 -> 2, 1536 -> 4 (gap, 3), 4096 -> 8, 4608 -> 12 (gap, 9), 6144 -> 12; 256 -> 1, 1160 -> 4 and 3072 -> 6 are in
      tests/test_hip_magi_block.py.
Every op keeps the bar of its existing oracle test.  Nine rows: the third workgroup has one busy wave and three idle ones."""
import pytest
import torch

import quant_oracle as Q
import wan_oracle as O
from util import assert_bf16_parity, pair_modulus

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROWS = 9
NORM_WIDTHS = [8, 512, 520, 1024, 2560, 3072, 3584, 4096, 4608, 5120]
QUANT_WIDTHS = [8, 512, 520, 1024, 2048, 3072, 5120, 5632, 9216, 9224, 12288]
GATE_WIDTHS = [520, 1024, 1536, 4096, 4608, 6144]


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def gpu(t):
    return t.cuda()


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def window(t, col0, fill):
    """(buffer, view): `t` as the column window [col0, col0 + cols) of a wider device buffer filled with `fill` — NaN around an input
    (a read outside the window poisons the result), a finite sentinel around an output (a write outside it is seen)."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + col0 + 40), fill, dtype=t.dtype, device="cuda")      # the row stride depends on col0
    view = buf[:, col0:col0 + cols]
    view.copy_(t)
    return buf, view


def margins_intact(buf, col0, cols, fill):
    return bool((buf[:, :col0] == fill).all()) and bool((buf[:, col0 + cols:] == fill).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# a. LayerNorm and RMSNorm on every rung and gap
def _offset_rows(g, dim):
    """2 * randn rows with means -3, -2.25 .. 3 (row 4: zero mean).  A lane of a chunk beyond `dim` holds zeros: left inside the
    squared deviations it adds mean^2 each, which zero-mean rows would hide (1e-4 of the variance) and these rows do not (0.03 to
    0.2 of it per unit of mean^2 at the ragged and gap widths)."""
    return (2.0 * torch.randn(1, ROWS, dim, generator=g) + 0.75 * (torch.arange(float(ROWS)) - 4).view(1, ROWS, 1)).to(BF)


@pytest.mark.parametrize("dim", NORM_WIDTHS)
def test_layernorm_every_rung_and_gap(ops, dim):
    g = torch.Generator().manual_seed(dim)
    rpg, groups = 3, ROWS // 3
    report = dim == NORM_WIDTHS[-1]
    x = _offset_rows(g, dim)
    assert_bf16_parity(ops.layernorm(gpu(x), 1e-6), O.layer_norm(x, 1e-6), max_ulp=1, what=f"LN plain {dim}", report=report)
    w, b = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF), (0.1 * torch.randn(dim, generator=g)).to(BF)
    assert_bf16_parity(ops.layernorm(gpu(x), 1e-6, gamma=gpu(w), beta=gpu(b)), O.layer_norm(x, 1e-6, w, b), max_ulp=1,
                       what=f"LN affine {dim}", report=report)
    mod = rnd(g, groups, 6, dim, scale=0.5)
    e = mod.unsqueeze(0).chunk(6, dim=2)
    for shift_slot, scale_slot in ((0, 1), (3, 4)):
        ref = O.modulate(O.layer_norm(x, 1e-6), e[scale_slot], e[shift_slot], groups)
        got = ops.layernorm(gpu(x), 1e-6, mod=gpu(mod), shift_slot=shift_slot, scale_slot=scale_slot, rows_per_group=rpg)
        assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, what=f"AdaLN {dim} slots {shift_slot},{scale_slot}", report=report)


@pytest.mark.parametrize("dim", NORM_WIDTHS)
def test_rmsnorm_every_rung_and_gap(ops, dim):
    g = torch.Generator().manual_seed(dim)
    x = rnd(g, ROWS, dim, scale=2.0)
    w = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    assert_bf16_parity(ops.rmsnorm(gpu(x), gpu(w), 1e-6), O.rms_norm(x, w, 1e-6), max_ulp=2, what=f"RMSNorm {dim}",
                       report=dim == NORM_WIDTHS[-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the per-token quantiser on every rung, gap and the generic loop
def _quant_rows(K, fmt):
    """The special rows of test_quant_per_token_bit_exact (tests/test_hip_quant.py), seeded from the width."""
    g = torch.Generator().manual_seed(K + fmt)
    x = rnd(g, ROWS, K, scale=3.0)
    x[1] = 0                                         # all-zero row -> scale 1, zeros
    x[2, 3] = 300.0                                  # outlier row
    x[3] = x[3] * 1e-30                              # tiny scale: the hoisted-reciprocal division must fall back
    x[4] = x[4] * 1e30                               # huge scale
    x[5, : K // 2] = (torch.arange(K // 2) % 255 - 127).to(BF)   # integers: exact quotients and .5 ties after the scale
    x[5, 0] = 254.0
    return x


@pytest.mark.parametrize("fmt", [Q.FP8, Q.INT8])
@pytest.mark.parametrize("K", QUANT_WIDTHS)
def test_quant_per_token_every_rung_gap_and_generic_loop(ops, K, fmt):
    x = _quant_rows(K, fmt)
    q, s = ops.quant_per_token(gpu(x), fmt)
    _, s_ref = Q.quantize_rows(x, fmt)
    assert torch.equal(s.cpu(), s_ref), "per-token scales must be bit-exact (fp32 abs-max / QMAX)"
    assert torch.equal(q.cpu(), Q.quantized_bytes(x, fmt)), "quantised bytes must be bit-exact"


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the gate-norm ladder
def _gate_case(dim):
    """The inputs of test_gate_norm_residual_vs_oracle with x and the gate shifted by one, so that the gated row x * gate has a mean
    (about 0.6, against a spread of about 1) and the masking of the idle chunks in the statistics shows (see _offset_rows)."""
    g = torch.Generator().manual_seed(dim)
    x = (torch.randn(ROWS, dim, generator=g) + 1.0).to(BF)
    res = torch.randn(ROWS, dim, generator=g).to(BF)
    gate = torch.tanh(torch.randn(3, 2 * dim, generator=g) + 1.0).to(BF)
    cmap = (torch.arange(ROWS) * 3 // ROWS).to(torch.int32)
    w, b = 0.1 * torch.randn(dim, generator=g), 0.1 * torch.randn(dim, generator=g)

    def ref(half):
        t = x.float() * gate[:, half * dim:(half + 1) * dim].float()[cmap.long()]
        return (torch.nn.functional.layer_norm(t, (dim,), w + 1, b, 1e-6) + res.float()).to(BF)
    return x, res, gate, cmap, w, b, ref


@pytest.mark.parametrize("dim", GATE_WIDTHS)
def test_gate_norm_residual_ladder(ops, dim):
    x, res, gate, cmap, w, b, ref = _gate_case(dim)
    for half in (0, 1):
        got = ops.magi_gate_norm_residual(gpu(x), gpu(res), gpu(cmap), gpu(gate)[:, half * dim:(half + 1) * dim], gpu(w), gpu(b), 1e-6,
                                          True)
        assert_bf16_parity(got, ref(half), max_ulp=1, floor=1.0, what=f"bias_modulate_add {dim} half {half}",
                           report=dim == GATE_WIDTHS[-1])


@pytest.mark.parametrize("dim", [520, 4608])
def test_gate_norm_residual_column_windows(ops, dim):
    """x, residual and out as column windows of wider buffers (three different row strides): NaN around the inputs, a sentinel around
    the output, which must stay intact — on a ragged width and on a gap width, whose idle chunks re-read column 0 of the window."""
    x, res, gate, cmap, w, b, ref = _gate_case(dim)
    _, xw = window(x, 8, float("nan"))
    _, rw = window(res, 16, float("nan"))
    obuf, ow = window(torch.zeros(ROWS, dim, dtype=BF), 24, 7.0)
    got = ops.magi_gate_norm_residual(xw, rw, gpu(cmap), gpu(gate)[:, dim:], gpu(w), gpu(b), 1e-6, True, out=ow)
    assert got.data_ptr() == ow.data_ptr()
    assert_bf16_parity(ow, ref(1), max_ulp=1, floor=1.0, what=f"bias_modulate_add {dim}, windows")
    assert margins_intact(obuf, 24, dim, 7.0), "columns outside the output window were written"


# ---------------------------------------------------------------------------------------------------------------------------------
# d. RoPE beyond chunk 0
GRID, START_FRAME = (3, 4, 6), 5


def _rope_case(ops, heads, hd, ws, rank):
    """Inputs, launch and oracle of one append: (rows, qkv on the device, wk, rope, local_start, cap, q_out, kc, vc, rq, rk, v)."""
    dim = heads * hd
    f, h, w = GRID
    hw_local = h * w // ws
    rows = f * hw_local
    g = torch.Generator().manual_seed(dim + ws)
    qkv = rnd(g, rows, 3 * dim, scale=2.0)
    wq = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    wk = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    freqs = O.rope_freqs(hd)
    q, k, v = qkv.split(dim, dim=1)
    rq = O.causal_rope_apply(O.rms_norm(q, wq, 1e-6).view(1, rows, heads, hd), GRID, freqs, START_FRAME, ws, rank)[0]
    rk = O.causal_rope_apply(O.rms_norm(k, wk, 1e-6).view(1, rows, heads, hd), GRID, freqs, START_FRAME, ws, rank)[0]
    cap, local_start = rows * 2 + 5, rows // 2 + 3
    kc = torch.zeros(cap, heads, hd, dtype=BF, device="cuda")
    vc = torch.zeros(cap, heads, hd, dtype=BF, device="cuda")
    rope = ops.RopeGridSpec(torch.view_as_real(freqs).contiguous().cuda(), START_FRAME, h, w, rank * hw_local, hw_local)
    qkv_g, wk_g = gpu(qkv), gpu(wk)
    qo = ops.rmsnorm_rope_kv_append(qkv_g, gpu(wq), wk_g, 1e-6, rope, ops.KvCacheView(kc, vc), local_start, dim)
    return rows, qkv_g, wk_g, rope, local_start, cap, qo, kc, vc, rq, rk, v


@pytest.mark.parametrize("ws,rank", [(1, 0), (2, 1)])
@pytest.mark.parametrize("heads,hd", [(12, 96), (4, 160), (3, 256), (20, 32)])
def test_rope_beyond_chunk_0(ops, heads, hd, ws, rank):
    """Rows wider than one 512-channel chunk at head sizes that do not divide 512 (96, 160: the general per-chunk rotation, whose
    in-head offset `col % head_dim` differs from the lane's own from chunk 1 on) and at two that do (256, 32: the shared pairs)."""
    rows, _, _, _, local_start, _, qo, kc, vc, rq, rk, v = _rope_case(ops, heads, hd, ws, rank)
    tag, report = f"{heads}x{hd} ws {ws}", (heads, ws) == (12, 1)
    assert_bf16_parity(qo.view(rows, heads, hd), rq, max_ulp=2, floor=1.0, scale=pair_modulus(rq), what=f"roped q {tag}", report=report)
    assert_bf16_parity(kc[local_start:local_start + rows], rk, max_ulp=2, floor=1.0, scale=pair_modulus(rk), what=f"cache K {tag}",
                       report=report)
    assert torch.equal(vc[local_start:local_start + rows].cpu(), v.reshape(rows, heads, hd)), "cache V must be bit-exact"
    for c in (kc, vc):
        assert float(c[:local_start].abs().max()) == 0 and float(c[local_start + rows:].abs().max()) == 0, "a slot outside the block was written"


@pytest.mark.parametrize("ws,rank", [(1, 0), (2, 1)])
def test_kv_push_equals_append_beyond_chunk_0(ops, ws, rank):
    """ifx_rmsnorm_rope_kv_push against the append on 12 heads of 96 channels (three chunks, general rotation): K and V bit for bit in
    both destinations, every other slot untouched."""
    heads, hd = 12, 96
    dim = heads * hd
    f, h, w = GRID
    frame_tokens = h * w
    hw_local = frame_tokens // ws
    hw_offset = rank * hw_local
    rows, qkv, wk, rope, local_start, _, _, kc, vc, _, _, _ = _rope_case(ops, heads, hd, ws, rank)
    cap = local_start + f * frame_tokens + 5
    dest = [torch.zeros(cap, heads, hd, dtype=BF, device="cuda") for _ in range(4)]          # k0, v0, k1, v1
    ops.rmsnorm_rope_kv_push(qkv[:, dim:], wk, 1e-6, rope, [dest[0].data_ptr(), dest[2].data_ptr()],
                             [dest[1].data_ptr(), dest[3].data_ptr()], ops.KvCacheView(dest[0], dest[1]), local_start, frame_tokens,
                             hw_local, hw_offset, dim)
    r = torch.arange(rows, device="cuda")
    slots = local_start + (r // hw_local) * frame_tokens + hw_offset + r % hw_local
    rest = torch.ones(cap, dtype=torch.bool, device="cuda")
    rest[slots] = False
    for k_dst, v_dst in ((dest[0], dest[1]), (dest[2], dest[3])):
        assert torch.equal(k_dst[slots], kc[local_start:local_start + rows]), "pushed K differs from the appended K"
        assert torch.equal(v_dst[slots], vc[local_start:local_start + rows]), "pushed V differs from the appended V"
        assert torch.equal(v_dst[slots], qkv[:, 2 * dim:].reshape(rows, heads, hd))
        assert not k_dst[rest].any() and not v_dst[rest].any(), "a slot outside the shard's tokens was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# e. paged, strided append
def test_append_through_a_page_table_from_a_strided_qkv(ops):
    """72 rows appended from logical token 19 through a permuted table of 16-token pages (the block starts inside page 1, ends inside
    page 5 and crosses four page boundaries), read from a column window of a wider NaN-filled buffer (ld = 3*dim + 64): K and V at the host-computed
    slots bit-equal to the dense unpaged launch's, every other slot untouched, q bit-equal to that launch's."""
    heads, hd, rows, ps, local_start = 2, 128, 72, 16, 19
    dim = heads * hd
    g = torch.Generator().manual_seed(dim + rows)
    qkv = rnd(g, rows, 3 * dim, scale=2.0)
    wq, wk = gpu((1 + 0.1 * torch.randn(dim, generator=g)).to(BF)), gpu((1 + 0.1 * torch.randn(dim, generator=g)).to(BF))
    npg = 8
    perm = torch.randperm(npg, generator=g)
    rope = ops.RopeGridSpec(torch.view_as_real(O.rope_freqs(hd)).contiguous().cuda(), 2, 4, 6)
    kd, vd = (torch.zeros(npg * ps, heads, hd, dtype=BF, device="cuda") for _ in range(2))
    q_dense = ops.rmsnorm_rope_kv_append(gpu(qkv), wq, wk, 1e-6, rope, ops.KvCacheView(kd, vd), local_start, dim)
    buf = torch.full((rows, 3 * dim + 64), float("nan"), dtype=BF, device="cuda")
    win = buf[:, 8:8 + 3 * dim]
    win.copy_(qkv)
    kp, vp = (torch.full((npg * ps, heads, hd), 7.0, dtype=BF, device="cuda") for _ in range(2))
    q_paged = ops.rmsnorm_rope_kv_append(win, wq, wk, 1e-6, rope, ops.KvCacheView(kp, vp, gpu(perm.to(torch.int32)), ps), local_start, dim)
    assert torch.equal(q_paged, q_dense), "q must not depend on the cache addressing or the row stride"
    t = torch.arange(local_start, local_start + rows)
    slots = perm[t // ps] * ps + t % ps
    assert torch.equal(kp.cpu()[slots], kd.cpu()[local_start:local_start + rows]), "K rows are not at their page-table slots"
    assert torch.equal(vp.cpu()[slots], vd.cpu()[local_start:local_start + rows]), "V rows are not at their page-table slots"
    assert torch.equal(vp.cpu()[slots], qkv[:, 2 * dim:].reshape(rows, heads, hd)), "cache V must be the projection's V"
    rest = torch.ones(npg * ps, dtype=torch.bool)
    rest[slots] = False
    assert bool((kp.cpu()[rest] == 7.0).all()) and bool((vp.cpu()[rest] == 7.0).all()), "a slot outside the block was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# f. strided norm and quantiser
@pytest.mark.parametrize("dim", [520, 2560])
def test_rmsnorm_row_strides(ops, dim):
    """ldx != ldy != dim: input and output are column windows; bit-equal to the dense call, margins of the output intact."""
    g = torch.Generator().manual_seed(dim)
    x = rnd(g, ROWS, dim, scale=2.0)
    w = gpu((1 + 0.1 * torch.randn(dim, generator=g)).to(BF))
    dense = ops.rmsnorm(gpu(x), w, 1e-6)
    _, xw = window(x, 8, float("nan"))
    obuf, ow = window(torch.zeros(ROWS, dim, dtype=BF), 16, 7.0)
    assert xw.stride(0) != ow.stride(0) and min(xw.stride(0), ow.stride(0)) > dim
    ops.rmsnorm(xw, w, 1e-6, out=ow)
    assert torch.equal(ow, dense)
    assert margins_intact(obuf, 16, dim, 7.0), "columns outside the output window were written"


@pytest.mark.parametrize("fmt", [Q.FP8, Q.INT8])
@pytest.mark.parametrize("K", [520, 2048, 9224])
def test_quant_per_token_row_strides(ops, K, fmt):
    """Windowed x and windowed q (a ragged width, a gap width and the generic loop): bytes and scales bit-equal to the dense call."""
    x = _quant_rows(K, fmt)
    q_dense, s_dense = ops.quant_per_token(gpu(x), fmt)
    _, xw = window(x, 8, float("nan"))
    qbuf, qw = window(torch.zeros(ROWS, K, dtype=torch.uint8), 16, 0xA5)
    q, s = ops.quant_per_token(xw, fmt, q=qw)
    assert q.data_ptr() == qw.data_ptr()
    assert torch.equal(qw, q_dense) and torch.equal(s, s_dense)
    assert margins_intact(qbuf, 16, K, 0xA5), "bytes outside the output window were written"


# ---------------------------------------------------------------------------------------------------------------------------------
# g. paged kv_roll
def test_kv_roll_through_a_page_table(ops):
    """The physical eviction shift that the model falls back to when a paged roll is not page aligned: sink 5, evicted 11, rolled 23
    over permuted pages of 8 tokens (source and destination spans overlap and none is a multiple of the page), expected result
    computed on the host by logical token."""
    g = torch.Generator().manual_seed(8)
    ps, npg, heads, hd = 8, 6, 2, 128
    sink, ev, rolled = 5, 11, 23
    k, v = rnd(g, npg * ps, heads, hd), rnd(g, npg * ps, heads, hd)
    perm = torch.randperm(npg, generator=g)
    t = torch.arange(npg * ps)
    slot = perm[t // ps] * ps + t % ps                      # logical token -> physical slot
    kk, vv = k.clone(), v.clone()
    kk[slot[sink:sink + rolled]] = k[slot[sink + ev:sink + ev + rolled]]
    vv[slot[sink:sink + rolled]] = v[slot[sink + ev:sink + ev + rolled]]
    kg, vg = gpu(k), gpu(v)
    ops.kv_roll(ops.KvCacheView(kg, vg, gpu(perm.to(torch.int32)), ps), sink, ev, rolled,
                torch.empty(rolled * heads * hd, dtype=BF, device="cuda"))
    assert torch.equal(kg.cpu(), kk) and torch.equal(vg.cpu(), vv)


# ---------------------------------------------------------------------------------------------------------------------------------
# h. offset rows
@pytest.mark.parametrize("dim", [520, 1160, 2560, 3584, 4608, 5120])
def test_layernorm_rows_with_a_large_mean(ops, dim):
    """Rows of 1024 + 8 * randn: the mean is 128 times the spread, so a one-pass variance E[x^2] - mean^2 in fp32 loses the spread to
    cancellation while the two-pass form of ln_stats does not.  Compared with the float64 evaluation rounded to bf16, with the cap on
    the mismatch FRACTION lifted (max_mismatch_frac = 1; the one-ULP element bound and the 1e-3 rel-L2 stay): at this magnitude bf16
    has steps of 8, the inputs take a handful of values and the normalised outputs sit on rounding ties, where the torch oracle
    alone differs from float64 in 2-5 % of the elements — the 0.02 cap would measure the ties, not the kernel.
    Which bound catches what (fp32 emulation on the CPU): a one-pass variance moves rstd by about 5e-4, a fraction of a bf16 step, so
    it stays inside the one-ULP element bound and is caught by the rel-L2 bound — 1.6e-3 to 1.7e-3 against 1e-3 at every width, where
    the oracle and a two-pass fp32 evaluation sit at <= 3.5e-4; bf16 cannot hold a row whose mean is much more than 128 times its
    spread, so this input is as far as that margin goes.  Zero lanes left inside the squared deviations (3584 and 4608, the gap
    widths of rungs 8 and 10, and every ragged width here) break the element bound outright."""
    g = torch.Generator().manual_seed(dim)
    x = (1024 + 8 * torch.randn(16, dim, generator=g)).to(BF)
    x64 = x.double()
    ref = ((x64 - x64.mean(-1, keepdim=True)) / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-6)).to(BF)
    assert_bf16_parity(ops.layernorm(gpu(x), 1e-6), ref, max_ulp=1, floor=1.0, max_mismatch_frac=1.0, what=f"LN offset rows {dim}",
                       report=dim == 5120)

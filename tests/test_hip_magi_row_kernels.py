"""GPU: the row kernels of inferix_amd/csrc/ifx_magi.hip against plain CPU references at the settings the MAGI layer runs and at
the edges of their loops (builders, references and rules: magi_rows_util.py; that the rules can fail: test_magi_rows_oracle.py).

  A  ifx_magi_head_prep: head counts that put several head types into one wave x every rotary width, q_scale, norm settings and
     planted heads, row counts, strided input and output windows, the all-to-all send order, layout 1, refusals of the C ABI;
  B  ifx_quant_static / ifx_quant_per_tensor, bit-exact: every finite bf16 value, every pass count of the 2048-column loop, windows,
     the strided grid of the abs-max kernel, the row-stride refusals;
  C  loop tails: ifx_silu_and_mul beyond its capped grid (the (row, chunk) carry), ifx_act_rows on every bf16 value,
     ifx_kv_split_rows with the second run in front of the first.

Found by B.2: with a divisor vector ifx_quant_static wrote 1.0 into `row_scale`, which the header reserves for divisor_len == 1;
the kernel now leaves it alone.  Nothing else failed: the quantisers agree with the references on every byte, subnormal inputs and
-0 included, and SiLU / tanh agree with torch on all 65 280 values bit for bit.

One `--durations=0` run of the whole suite on an MI355X: the 110 tests of this file 0.34 s together, the slowest 0.20 s
(test_silu_and_mul_beyond_the_capped_grid), the 22 CPU tests of test_magi_rows_oracle.py 0.14 s, the suite 296.3 s with them
(295.8 s without)."""
import pytest
import torch
import torch.nn.functional as F

import magi_rows_util as U
from magi_rows_util import BF, HD, NAN
from util import bf16_ulp_diff

pytestmark = pytest.mark.gpu
ROWS = 37
FORMATS = ("e4m3", "int8")
_SHARED = {}          # device results that several cases compare with, computed once


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def _fmt(name):
    from inferix_amd import _hip
    return _hip.IFX_Q_FP8_E4M3 if name == "e4m3" else _hip.IFX_Q_INT8


def _params(inp):
    return dict(rope=inp["rope"].cuda(), qn=[t.cuda() for t in inp["qn"]], kn=[t.cuda() for t in inp["kn"]],
                xn=[t.cuda() for t in inp["xn"]])


def dense_launch(ops, inp, q_scale=0.0, one_p=True, eps=U.EPS):
    """The plain layout-0 launch: contiguous input, q / qx [rows, hq, 128], k / v [rows, hk, 128] at row0 = 0."""
    rows, hq, hk = inp["rows"], inp["hq"], inp["hk"]
    q = torch.full((rows, hq * HD), 7.0, dtype=BF, device="cuda")
    qx = torch.full_like(q, 7.0)
    kc = torch.full((rows, hk, HD), 7.0, dtype=BF, device="cuda")
    vc = torch.full_like(kc, 7.0)
    ops.magi_head_prep(inp["mixed"].cuda(), layout=0, q_heads=hq, kv_heads=hk, eps=eps, layernorm_1p=one_p, k_out=kc, v_out=vc,
                       kv_head_stride=HD, ld_kv=hk * HD, q_out=q, qx_out=qx, q_scale=q_scale, **_params(inp))
    return dict(q=q.view(rows, hq, HD), qx=qx.view(rows, hq, HD), k=kc, v=vc)


def shared_dense(ops, rows, hq, hk, half=48):
    key = (rows, hq, hk, half)
    if key not in _SHARED:
        inp = U.head_prep_inputs(rows, hq, hk, half)
        got = dense_launch(ops, inp, q_scale=U.Q_PRESCALE)
        U.judge_head_prep(None, got, U.head_prep_reference(inp, U.Q_PRESCALE), what=f"dense {key}")
        _SHARED[key] = (inp, got)
    return _SHARED[key]


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ---- A. head prep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", U.ROPE_HALVES)
@pytest.mark.parametrize("hq,hk", U.HEAD_COUNTS)
def test_head_prep_head_counts_and_rotary_widths(ops, hq, hk, half):
    """A.1: 37 rows, the attention prescale, layernorm_1p.  (1, 1), (2, 1) and (3, 1) hold q, qx, k and v heads in one wave ((2, 1):
    6 slots, two idle 16-lane groups in the last wave); the rotary partner lane is half / 8 away, lanes at and behind 2 half pass."""
    inp = U.head_prep_inputs(ROWS, hq, hk, half)
    ref = U.head_prep_reference(inp, U.Q_PRESCALE)
    assert ops.attn_q_prescale(HD)[0] == U.Q_PRESCALE
    got = dense_launch(ops, inp, q_scale=ops.attn_q_prescale(HD)[0])
    U.judge_head_prep("A.1", got, ref, what=f"{hq}/{hk} half {half}")
    if half < 64:          # behind the rotary width: the LayerNorm alone
        for name in ("q", "k"):
            assert torch.equal(ref[name][..., 2 * half:], ref[name + "_ln"][..., 2 * half:])
            U.judge("A.1", got[name][..., 2 * half:], ref[name + "_ln"][..., 2 * half:], max_ulp=1, floor=1.0,
                    what=f"{hq}/{hk} half {half} {name} pass-through")
    U.report("A.1")


def test_head_prep_q_scale(ops):
    """A.2 at (3, 1), half 48: 0 means 1; 0.5 commutes with the single rounding (inputs of order 1, far from subnormals), so a second
    rounding of q would show; the prescale meets the oracle; k, qx and v do not see the scale."""
    inp = U.head_prep_inputs(ROWS, 3, 1, 48)
    runs = {s: dense_launch(ops, inp, q_scale=s) for s in (0.0, 1.0, 0.5, U.Q_PRESCALE)}
    assert _bits_equal(runs[0.0]["q"], runs[1.0]["q"]), "q_scale 0 must mean 1"
    assert _bits_equal(runs[0.5]["q"], (runs[1.0]["q"].float() * 0.5).to(BF)), "q_scale 0.5: q is rounded more than once"
    for s, got in runs.items():
        U.judge_head_prep("A.2", got, U.head_prep_reference(inp, s), what=f"q_scale {s}")
        for name in ("k", "qx", "v"):
            assert _bits_equal(got[name], runs[0.0][name]), (name, s)
    U.report("A.2")


@pytest.mark.parametrize("case", ["no_1p"] + list(U.PLANTS))
def test_head_prep_norm_settings(ops, case):
    """A.3 at (3, 1), half 48: layernorm_1p off; planted heads (one q, one qx, one k slot on three rows) of variance ~1.5e-5 (a
    kernel with eps = 1e-5 misses the bar there by ~30x), of variance 0 (finite, = the bias) and at 40 +- 0.4."""
    one_p = case != "no_1p"
    inp = U.head_prep_inputs(ROWS, 3, 1, 48, plant=case if one_p else None)
    got = dense_launch(ops, inp, q_scale=U.Q_PRESCALE, one_p=one_p)
    for name in ("q", "qx", "k"):
        assert bool(torch.isfinite(got[name].float()).all()), name
    U.judge_head_prep("A.3", got, U.head_prep_reference(inp, U.Q_PRESCALE, one_p=one_p), what=case)
    U.report("A.3")


@pytest.mark.parametrize("rows", [1, 2, 4, 333])
def test_head_prep_row_counts(ops, rows):
    """A.4 at (3, 1): two waves per row, so 1 row is half a block, 2 rows one block, 333 rows 167 blocks with a half-empty last one."""
    inp = U.head_prep_inputs(rows, 3, 1, 48)
    U.judge_head_prep("A.4", dense_launch(ops, inp, q_scale=U.Q_PRESCALE), U.head_prep_reference(inp, U.Q_PRESCALE), what=f"{rows} rows")
    U.report("A.4")


P_ROWS, P_HQ, P_HK, P_SLOTS = 333, 6, 2, 540


def _windowed_launch(ops, inp, **kv):
    """The launch of A.5: `mixed` is the column window [8, 8 + n 128) of a NaN buffer (ld_in = n 128 + 72), q / qx are windows of
    7.0-filled buffers; returns the two output buffers' views after checking that their margins still hold 7.0."""
    rows, hq, hk = inp["rows"], inp["hq"], inp["hk"]
    _, xv = U.window(inp["mixed"], 8, NAN, extra=64)
    assert xv.stride(0) == (2 * hq + 2 * hk) * HD + 72
    qbuf, qv = U.window(torch.zeros(rows, hq * HD, dtype=BF), 24, 7.0)
    xbuf, qxv = U.window(torch.zeros(rows, hq * HD, dtype=BF), 16, 7.0, extra=8)
    qv.fill_(7.0), qxv.fill_(7.0)
    ops.magi_head_prep(xv, layout=0, q_heads=hq, kv_heads=hk, eps=U.EPS, layernorm_1p=True, q_out=qv, qx_out=qxv, q_scale=U.Q_PRESCALE,
                       **kv, **_params(inp))
    assert U.margins_intact(qbuf, 24, hq * HD, 7.0) and U.margins_intact(xbuf, 16, hq * HD, 7.0), "a write outside the q / qx windows"
    return qv, qxv


@pytest.mark.parametrize("row0,split,row1", [(100, 200, 400), (0, P_ROWS, 0), (50, 0, 10), (300, 100, 5)])
def test_head_prep_placement_in_the_cache(ops, row0, split, row1):
    """A.5: strided input, output windows, and the two destination runs of the k / v rows in 7.0-filled cache planes — every split
    form of the store rule, (300, 100, 5) with the second run in front of the first.  Bits of the dense launch; all else still 7.0."""
    inp, dense = shared_dense(ops, P_ROWS, P_HQ, P_HK)
    kc = torch.full((P_SLOTS, P_HK, HD), 7.0, dtype=BF, device="cuda")
    vc = torch.full_like(kc, 7.0)
    qv, qxv = _windowed_launch(ops, inp, k_out=kc, v_out=vc, kv_head_stride=HD, ld_kv=P_HK * HD, row0=row0, split=split, row1=row1)
    assert _bits_equal(qv.reshape(P_ROWS, P_HQ, HD), dense["q"]) and _bits_equal(qxv.reshape(P_ROWS, P_HQ, HD), dense["qx"])
    dest = torch.cat([torch.arange(row0, row0 + split), torch.arange(row1, row1 + P_ROWS - split)]).cuda()
    assert dest.unique().numel() == P_ROWS and int(dest.max()) < P_SLOTS
    assert _bits_equal(kc[dest], dense["k"]) and _bits_equal(vc[dest], dense["v"])
    other = torch.ones(P_SLOTS, dtype=torch.bool, device="cuda")
    other[dest] = False
    assert bool((kc[other] == 7.0).all()) and bool((vc[other] == 7.0).all()), "cache rows outside the two runs were written"


@pytest.mark.parametrize("staging", ["head_major", "row_major"])
def test_head_prep_placement_in_the_staging_buffers(ops, staging):
    """A.5, the all-to-all staging layouts of dit.py: K | V of one kv head side by side, `head_major` [hk, rows, 256]
    (kv_head_stride = rows 256, ld_kv = 256) and `row_major` [rows, hk, 256] (kv_head_stride = 256, ld_kv = hk 256)."""
    inp, dense = shared_dense(ops, P_ROWS, P_HQ, P_HK)
    if staging == "head_major":
        buf = torch.full((P_HK, P_ROWS, 2 * HD), 7.0, dtype=BF, device="cuda")
        kv = dict(kv_head_stride=P_ROWS * 2 * HD, ld_kv=2 * HD)
        rows_first = buf.transpose(0, 1)
    else:
        buf = torch.full((P_ROWS, P_HK, 2 * HD), 7.0, dtype=BF, device="cuda")
        kv = dict(kv_head_stride=2 * HD, ld_kv=P_HK * 2 * HD)
        rows_first = buf
    qv, qxv = _windowed_launch(ops, inp, k_out=buf, v_out=buf.view(-1)[HD:], **kv)
    assert _bits_equal(qv.reshape(P_ROWS, P_HQ, HD), dense["q"]) and _bits_equal(qxv.reshape(P_ROWS, P_HQ, HD), dense["qx"])
    assert _bits_equal(rows_first[..., :HD], dense["k"]) and _bits_equal(rows_first[..., HD:], dense["v"])


@pytest.mark.parametrize("hq,hk,q_group", [(24, 8, 3), (6, 2, 3), (6, 2, 2), (6, 2, 6)])
def test_head_prep_q_in_send_order(ops, hq, hk, q_group):
    """A.6: q written as [hq / q_group, rows, q_group 128], the head -> rank all-to-all's send order: the plain launch, permuted;
    qx, k and v as before."""
    inp, dense = shared_dense(ops, ROWS, hq, hk)
    groups = hq // q_group
    q_send = torch.full((groups, ROWS, q_group * HD), 7.0, dtype=BF, device="cuda")
    qx = torch.full((ROWS, hq * HD), 7.0, dtype=BF, device="cuda")
    kc = torch.full((ROWS, hk, HD), 7.0, dtype=BF, device="cuda")
    vc = torch.full_like(kc, 7.0)
    ops.magi_head_prep(inp["mixed"].cuda(), layout=0, q_heads=hq, kv_heads=hk, eps=U.EPS, layernorm_1p=True, k_out=kc, v_out=vc,
                       kv_head_stride=HD, ld_kv=hk * HD, q_out=q_send, qx_out=qx, q_scale=U.Q_PRESCALE, q_group=q_group, **_params(inp))
    want = dense["q"].reshape(ROWS, groups, q_group * HD).transpose(0, 1)
    assert _bits_equal(q_send, want), "q in send order differs from the plain launch"
    assert _bits_equal(qx.view(ROWS, hq, HD), dense["qx"]) and _bits_equal(kc, dense["k"]) and _bits_equal(vc, dense["v"])


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("hk", [1, 3, 8])
def test_head_prep_layout_1(ops, hk, rows):
    """A.7: the caption keys / values, hk x (kx | v) per row, read from a NaN-framed window: kx through the bf16 LayerNorm, v a copy.
    hk = 1 is half a wave, hk = 3 a wave and a half."""
    g = torch.Generator().manual_seed(hk * 100 + rows)
    kvx = torch.randn(rows, 2 * hk * HD, generator=g).to(BF)
    xn = ((0.1 * torch.randn(HD, generator=g)).to(BF), (0.1 * torch.randn(HD, generator=g)).to(BF))
    _, xv = U.window(kvx, 8, NAN)
    kx = torch.full((rows + 2, hk, HD), 7.0, dtype=BF, device="cuda")
    vx = torch.full_like(kx, 7.0)
    ops.magi_head_prep(xv, layout=1, q_heads=0, kv_heads=hk, eps=U.EPS, layernorm_1p=True, k_out=kx, v_out=vx, kv_head_stride=HD,
                       ld_kv=hk * HD, row0=1, xn=[t.cuda() for t in xn])
    kx_ref, v_ref = U.kx_reference(kvx, xn, hk)
    U.judge("A.7", kx[1:rows + 1], kx_ref, max_ulp=1, floor=0.05, what=f"kx hk {hk} rows {rows}")
    assert _bits_equal(vx[1:rows + 1], v_ref)
    for t in (kx, vx):
        assert bool((t[0] == 7.0).all()) and bool((t[rows + 1] == 7.0).all())
    U.report("A.7")


def test_head_prep_refusals_through_the_c_abi(ops):
    """A.8: the descriptor built directly; each refusal differs from an accepted descriptor in one field."""
    import ctypes as C
    from inferix_amd import _hip
    rows, hq, hk = 4, 24, 8
    n = 2 * hq + 2 * hk
    mixed = torch.zeros(rows, n * HD, dtype=BF, device="cuda")
    rope = torch.zeros(rows, 2 * 72, device="cuda")
    f32 = torch.zeros(4, HD, device="cuda")
    b16 = torch.zeros(2, HD, dtype=BF, device="cuda")
    q = torch.zeros(rows, hq * HD, dtype=BF, device="cuda")
    qx = torch.zeros_like(q)
    kc = torch.zeros(rows, hk, HD, dtype=BF, device="cuda")
    vc = torch.zeros_like(kc)

    def call(**over):
        d = _hip.MagiHeadPrepDesc()
        d.in_, d.ld_in, d.rows, d.layout, d.q_heads, d.kv_heads, d.head_dim = mixed.data_ptr(), n * HD, rows, 0, hq, hk, HD
        d.rope, d.rope_half = rope.data_ptr(), 48
        d.qn_w, d.qn_b, d.kn_w, d.kn_b = (f32[i].data_ptr() for i in range(4))
        d.xn_w, d.xn_b = b16[0].data_ptr(), b16[1].data_ptr()
        d.eps, d.layernorm_1p, d.q_scale = 1e-6, 1, 1.0
        d.q_out, d.ld_q, d.qx_out, d.ld_qx = q.data_ptr(), hq * HD, qx.data_ptr(), hq * HD
        d.k_out, d.v_out, d.ld_kv, d.kv_head_stride = kc.data_ptr(), vc.data_ptr(), hk * HD, HD
        d.row0, d.split, d.row1 = 0, rows, 0
        for name, value in over.items():
            setattr(d, name, value)
        _hip.check(_hip.load().ifx_magi_head_prep(C.byref(d), torch.cuda.current_stream().cuda_stream), "ifx_magi_head_prep")

    call()
    call(q_group=3, ld_q=3 * HD, q_group_stride=rows * 3 * HD)
    for over, match in ((dict(head_dim=64), r"head_dim 64"), (dict(rope_half=4), r"rope_half \(4\)"), (dict(rope_half=72), r"rope_half \(72\)"),
                        (dict(q_group=5, ld_q=5 * HD, q_group_stride=rows * 5 * HD), r"q_group 5"),
                        (dict(ld_q=hq * HD - 8), r"q row strides"), (dict(ld_in=n * HD - 8), r"ld_in")):
        with pytest.raises(_hip.HipKernelError, match=match):
            call(**over)
    torch.cuda.synchronize()


# ---- B. the static and per-tensor quantisers, byte for byte -------------------------------------------------------------------------------
def _byte_diff(got, ref, x=None):
    """'' when equal; otherwise the count of differing bytes, by input class when the input is given."""
    got = got.cpu()
    bad = got != ref
    if not bool(bad.any()):
        return ""
    msg = f"{int(bad.sum())} of {bad.numel()} bytes differ"
    if x is not None:
        bits = x.cpu().view(torch.int16).to(torch.int32) & 0xFFFF
        sub = ((bits & 0x7F80) == 0) & ((bits & 0x7F) != 0)
        msg += (f" ({int((bad & sub).sum())} at subnormal inputs, {int((bad & (bits == 0x8000)).sum())} at -0, "
                f"{int((bad & (bits == 0)).sum())} at +0, {int((bad & ~sub & ((bits & 0x7FFF) != 0)).sum())} at normal inputs)")
    return msg


@pytest.mark.parametrize("via_bf16", [True, False])
@pytest.mark.parametrize("fmt", FORMATS)
def test_quant_static_every_finite_bf16_value(ops, fmt, via_bf16):
    """B.1: all 65 280 finite bf16 patterns (subnormals, both zeros, up to 3.39e38) under five single divisors and one vector
    cycling through them.  Ties, saturation, e4m3 subnormals and -0 are all among them; divisors 0.03, 1000 (e4m3) and 3.0 (int8)
    tell the bf16 intermediate from the direct cast (test_magi_rows_oracle.py)."""
    x = U.all_finite_bf16()
    xd = x.cuda()
    for d in [torch.tensor([v]) for v in U.DIVISORS] + [U.cycling_divisor(544)]:
        got = ops.quant_static(xd, d.cuda(), _fmt(fmt), via_bf16=via_bf16)
        diff = _byte_diff(got, U.quant_reference(x, d, fmt, via_bf16), x)
        assert not diff, f"{fmt} via_bf16 {via_bf16} divisor {d[:5].tolist()}: {diff}"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("K", [8, 512, 520, 1160, 2048, 2056, 4104, 6144])
def test_quant_static_width_classes(ops, K, fmt):
    """B.2: 9 rows (three blocks, the last with one row).  One pass of the loop takes four 512-column chunks: 2056 is a second pass
    with one busy lane, 4104 a third.  Divisor [K] and [1]; row_scale is filled with divisor[0] for [1] and left alone for [K]."""
    x, dvec = U.quant_rows(9, K)
    xd = x.cuda()
    for via in (True, False):
        for d in (dvec, dvec[3:4].clone()):
            rs = torch.full((9,), -7.0, device="cuda")
            got = ops.quant_static(xd, d.cuda(), _fmt(fmt), via_bf16=via, row_scale=rs)
            diff = _byte_diff(got, U.quant_reference(x, d, fmt, via))
            assert not diff, f"K {K} {fmt} via_bf16 {via} divisor [{d.numel()}]: {diff}"
            want = d[0] if d.numel() == 1 else torch.tensor(-7.0)
            assert torch.equal(rs.cpu(), want.expand(9)), "row_scale"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("K", [520, 2056])
def test_quant_static_in_windows(ops, K, fmt):
    """B.3: x inside a NaN frame, q inside a 0x5A byte frame (ldq > K): the dense launch's bytes, margins intact."""
    x, dvec = U.quant_rows(9, K)
    _, xv = U.window(x, 16, NAN)
    for via in (True, False):
        for d in (dvec.cuda(), dvec[3:4].cuda()):
            dense = ops.quant_static(x.cuda(), d, _fmt(fmt), via_bf16=via)
            assert not _byte_diff(dense, U.quant_reference(x, d.cpu(), fmt, via))
            qbuf, qv = U.window(torch.zeros(9, K, dtype=torch.uint8), 24, 0x5A)
            qv.fill_(0x5A)
            ops.quant_static(xv, d, _fmt(fmt), via_bf16=via, q=qv)
            assert torch.equal(qv, dense) and U.margins_intact(qbuf, 24, K, 0x5A), (K, fmt, via, d.numel())


def _big_rows():
    if "big" not in _SHARED:
        g = torch.Generator().manual_seed(1030)
        _SHARED["big"] = torch.randn(1030, 2056, generator=g).to(BF)
    return _SHARED["big"]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("peak", [96.0, -96.0])
def test_quant_per_tensor_beyond_the_first_grid_pass(ops, peak, fmt):
    """B.4: 1030 x 2056 = 264 710 chunks, more than the 1024 x 256 lanes of the abs-max kernel's capped grid; max |x| sits at the
    last element of the last row, which only the strided second pass reaches.  Scale amax / QMAX exact, bytes by the definition."""
    x = _big_rows().clone()
    x[-1, -1] = peak
    assert float(x[:-1].float().abs().max()) < 8.0
    q, s = ops.quant_per_tensor(x.cuda(), _fmt(fmt))
    q_ref, s_ref = U.per_tensor_reference(x, fmt)
    assert float(s_ref) == float(torch.tensor(96.0) / U.QMAX[fmt])
    assert torch.equal(s.cpu(), s_ref.expand(1030)), (float(s[0]), float(s[-1]), float(s_ref))
    assert not _byte_diff(q, q_ref)


@pytest.mark.parametrize("fmt", FORMATS)
def test_quant_per_tensor_window_and_zero(ops, fmt):
    """B.4: a (9, 520) window in a frame of 3e38 (finite: fmaxf would drop a NaN, an over-read of the abs-max kernel would not show):
    the scale comes from the window alone.  An all-zero tensor: scale 1, zero bytes."""
    x, _ = U.quant_rows(9, 520)
    _, xv = U.window(x, 16, 3e38)
    qbuf, qv = U.window(torch.zeros(9, 520, dtype=torch.uint8), 24, 0x5A)
    q, s = ops.quant_per_tensor(xv, _fmt(fmt), q=qv)
    q_ref, s_ref = U.per_tensor_reference(x, fmt)
    assert torch.equal(s.cpu(), s_ref.expand(9)), (float(s[0]), float(s_ref))
    assert not _byte_diff(qv, q_ref) and U.margins_intact(qbuf, 24, 520, 0x5A)
    z = torch.zeros(9, 520, dtype=BF, device="cuda")
    q, s = ops.quant_per_tensor(z, _fmt(fmt))
    assert torch.equal(s.cpu(), torch.ones(9)) and int(q.count_nonzero()) == 0


def test_quantisers_refuse_row_strides_below_k(ops):
    """B.5: with ldq < K rows would overwrite each other (ldx < K: rows read twice); refused like ifx_silu_and_mul does."""
    from inferix_amd import _hip
    K = 520
    x = torch.zeros(9 * K, dtype=BF, device="cuda")
    q = torch.zeros(9 * K, dtype=torch.uint8, device="cuda")
    d = torch.ones(1, device="cuda")
    narrow = lambda t: t.as_strided((9, K), (K - 8, 1))
    wide = lambda t: t.as_strided((9, K), (K, 1))
    ops.quant_static(wide(x), d, _fmt("e4m3"), via_bf16=True, q=wide(q))
    ops.quant_per_tensor(wide(x), _fmt("int8"), q=wide(q))
    for xs, qs, match in ((narrow(x), wide(q), r"ldx \(512\)"), (wide(x), narrow(q), r"ldq \(512\)")):
        with pytest.raises(_hip.HipKernelError, match="ifx_quant_static.*" + match):
            ops.quant_static(xs, d, _fmt("e4m3"), via_bf16=True, q=qs)
        with pytest.raises(_hip.HipKernelError, match="ifx_quant_per_tensor.*" + match):
            ops.quant_per_tensor(xs, _fmt("int8"), q=qs)


# ---- C. loop tails ------------------------------------------------------------------------------------------------------------------------
def test_silu_and_mul_beyond_the_capped_grid(ops):
    """C.1: 3700 x 1160 = 536 500 chunks on 2048 x 256 = 524 288 lanes (dr = 3615, dc = 113): lanes 0 .. 12 211 run the loop body a
    second time, those with chunk >= 32 through the carry of (row, chunk).  The bar of test_hip_gated_kernels.py (2 ULP, <= 2 % off);
    q == ifx_quant_static of the bf16 result."""
    rows, f = 3700, 1160
    assert rows * (f // 8) - 2048 * 256 == 12212 and divmod(2048 * 256, f // 8) == (3615, 113)
    g = torch.Generator().manual_seed(rows + f)
    x = (2.0 * torch.randn(rows, 2 * f, generator=g)).to(BF)
    ref = F.silu(x[:, :f]) * x[:, f:]          # the oracle chain (magi_block_oracle.py): two bf16 roundings
    xd = x.cuda()
    y = ops.silu_and_mul(xd)
    U.judge("C.1", y, ref, max_ulp=2, floor=1.0, what="silu_and_mul 3700 x 1160")
    U.judge("C.1", y[3615:], ref[3615:], max_ulp=2, floor=1.0, what="silu_and_mul, the rows of the second iteration")
    div = (0.03 * (1 + 0.5 * torch.rand(f, generator=g))).cuda()
    for d in (div, div[:1].clone()):
        y2, q = ops.silu_and_mul(xd, out=torch.empty_like(y), quant_divisor=d)
        assert torch.equal(y2, y)
        assert torch.equal(q, ops.quant_static(y, d, _fmt("e4m3"), via_bf16=True)), d.numel()
    assert not _byte_diff(q, U.quant_reference(y.cpu(), div[:1].cpu(), "e4m3", True))
    U.report("C.1")


@pytest.mark.parametrize("mode", ["silu", "tanh"])
@pytest.mark.parametrize("n", [1, 255, 257, 65280])
def test_act_rows_sizes_and_every_bf16_value(ops, n, mode):
    """C.2: one lane, a block less one, a block and one, and every finite bf16 value.  The existing bar (max_ulp = 1) on the whole
    tensor and, because its floor follows the tensor RMS (~1e37 over all values), on each sign x magnitude band as well."""
    from inferix_amd import _hip
    x = U.all_finite_bf16().flatten()
    if n < 65280:          # values of every magnitude the gates see, both signs
        x = x[torch.randperm(65280, generator=torch.Generator().manual_seed(n))[:n]].clone()
    ref = U.act_reference(x, mode)
    out = torch.full((n + 8,), 7.0, dtype=BF, device="cuda")
    got = ops.act_rows(x.cuda(), _hip.IFX_ACT_SILU if mode == "silu" else _hip.IFX_ACT_TANH, out=out[:n])
    assert bool((out[n:] == 7.0).all())
    U.judge("C.2", got, ref, max_ulp=1, floor=0.05, what=f"{mode} n {n}")
    if n == 65280:
        for name, m in U.act_bands(x):
            if not bool(ref[m].float().any()):          # silu below -128: x / (1 + inf) = -0 throughout, no scale to take an ULP at
                assert not bool(got.cpu()[m].float().any()), f"{mode} band {name}: the reference is zero throughout"
                continue
            U.judge("C.2", got.cpu()[m], ref[m], max_ulp=1, floor=0.05, what=f"{mode} band {name}")
        d = bf16_ulp_diff(got.cpu(), ref)
        print(f"{mode}: {int((d > 0).sum())} of 65280 values differ, largest bit-pattern distance {int(d.max())}")
    U.report("C.2")


@pytest.mark.parametrize("n,heads,row0,split,row1,slots", [(50, 3, 30, 0, 5, 80), (1, 1, 3, 1, 0, 8), (1, 2, 0, 0, 6, 8),
                                                           (20, 8, 4, 9, 40, 64)])
def test_kv_split_rows_more_cases(ops, n, heads, row0, split, row1, slots):
    """C.3, next to the four cases of test_kv_split_rows_is_the_four_copies: split = 0 with the run in front of row0, one row (in
    either run), eight heads."""
    g = torch.Generator().manual_seed(n + heads)
    kv = torch.randn(n, heads, 2 * HD, generator=g).to(BF).cuda()
    kc = torch.full((slots, heads, HD), 3.0, dtype=BF, device="cuda")
    vc = torch.full((slots, heads, HD), 5.0, dtype=BF, device="cuda")
    kr, vr = kc.clone(), vc.clone()
    kr[row0:row0 + split], vr[row0:row0 + split] = kv[:split, :, :HD], kv[:split, :, HD:]
    kr[row1:row1 + n - split], vr[row1:row1 + n - split] = kv[split:, :, :HD], kv[split:, :, HD:]
    ops.kv_split_rows(kv, kc, vc, row0, split, row1)
    assert torch.equal(kc, kr) and torch.equal(vc, vr), (n, heads, row0, split, row1)

"""Input builders, CPU references and the judging rules of the MAGI row-kernel tests (inferix_amd/csrc/ifx_magi.hip):
test_magi_rows_oracle.py proves on the CPU that the head-prep rule accepts an fp32 restatement of the kernel's arithmetic and rejects
every single-step departure from it; test_hip_magi_row_kernels.py applies the rules to the HIP launches.

Head prep.  A fused projection row holds 128-wide head slots [hq q | hq qx | hk k | hk v]; the kernel gives one 16-lane group to a
slot and four slots to a wave, so with hq = 1, 2 or 3 on hk = 1 a wave holds several head TYPES at once.  The reference of q is
`MB.fused_layer_norm` on fp32, `MB.apply_rotary` kept in fp32, x float32(q_scale), ONE cast to bf16 (k: the same without the scale);
qx / kx are the bf16 module (`w + 1` in bf16); v is a copy.  The bars are those of test_hip_magi_block.py::test_head_prep_vs_oracle.

Quantisers.  `quant_reference` is ifx_quant_static as include/inferix_hip.h words it, in torch on the CPU, compared byte for byte."""
import functools
import math

import torch
import torch.nn.functional as F

import magi_block_oracle as MB
from util import assert_bf16_parity, rel_l2

BF = torch.bfloat16
HD = 128
NAN = float("nan")
EPS = 1e-6
ROPE_HALVES = (8, 16, 24, 32, 40, 48, 56, 64)
HEAD_COUNTS = ((1, 1), (2, 1), (3, 1), (6, 2), (24, 8))
Q_PRESCALE = (HD ** -0.5) * 1.4426950408889634          # hip_ops.attn_q_prescale(128)[0], what dit.py passes as q_scale
QMAX = {"e4m3": 448.0, "int8": 127.0}
DIVISORS = (1.0, 0.03, 3.0, 2.0 ** -10, 1000.0)


# ---- the judging rule, with the figures it judged kept per group ----------------------------------------------------------------------
FIGURES = {}          # group -> [worst element error / bound, worst mismatch fraction, worst rel L2 / bound, comparisons]


def parity_figures(got, ref, *, max_ulp, floor, rel=1e-3):
    """(element error / bound, mismatch fraction, rel L2 / bound): the three numbers `assert_bf16_parity` (util.py) judges."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    g, r0 = got.double(), ref.double()
    rms = float(r0.pow(2).mean().sqrt())
    tol = max_ulp * 2.0 ** -7 * torch.maximum(r0.abs(), torch.tensor(floor * rms, dtype=torch.float64))
    diff = (g - r0).abs()
    worst = float((diff / tol).max()) if bool(torch.isfinite(g).all()) else math.inf
    return worst, float((diff > 0).double().mean()), rel_l2(got, ref) / rel


def judge(group, got, ref, *, max_ulp, floor, what, max_mismatch_frac=0.02, rel=1e-3):
    """`assert_bf16_parity` with its figures recorded under `group` first (a failing comparison shows in the record too)."""
    f = parity_figures(got, ref, max_ulp=max_ulp, floor=floor, rel=rel)
    if group is not None:
        w = FIGURES.setdefault(group, [0.0, 0.0, 0.0, 0])
        w[0], w[1], w[2], w[3] = max(w[0], f[0]), max(w[1], f[1]), max(w[2], f[2]), w[3] + 1
    assert_bf16_parity(got, ref, max_ulp=max_ulp, floor=floor, max_mismatch_frac=max_mismatch_frac, rel=rel, what=what)
    return f


def report(group):
    w = FIGURES.get(group)
    if w is not None:
        print(f"[{group}] over {w[3]} comparisons: worst element error {w[0]:.3f} of its bound, worst mismatch fraction {w[1]:.5f} "
              f"(bound 0.02), worst rel L2 {w[2]:.3f} of its bound")


def judge_head_prep(group, got, ref, what="", only=None):
    """The rule of part A on the outputs present in `got`: q / k at 1 ULP with floor 1 (LayerNorm + rotary: results of cancellations),
    qx / kx at 1 ULP with floor 0.05 (a pure normalisation), v a copy; at most 2 % of the elements off, rel L2 <= 1e-3."""
    for name in ("q", "k", "qx", "kx"):
        if name in got and (only is None or name in only):
            judge(group, got[name], ref[name], max_ulp=1, floor=1.0 if name in ("q", "k") else 0.05, what=f"{what} {name}")
    if "v" in got and (only is None or "v" in only):
        assert torch.equal(got["v"].detach().cpu().view(torch.int16), ref["v"].view(torch.int16)), f"{what} v is a copy"


# ---- head prep: inputs ------------------------------------------------------------------------------------------------------------------
PLANTS = ("low_variance", "constant", "offset")


def plant_head(kind, g):
    """One 128-channel head that stresses the statistics: `low_variance` = 1 + 2^-7 {0, 1} (variance ~1.5e-5: eps = 1e-6 is 6 % of it,
    1e-5 would be 40 %); `constant` (variance 0: rstd = eps^-1/2, the result is the bias); `offset` = 40 +- 0.4 (the mean dwarfs the
    deviations: a one-pass E[x^2] - mean^2 loses them)."""
    if kind == "low_variance":
        return (1.0 + 2.0 ** -7 * torch.randint(0, 2, (HD,), generator=g).float()).to(BF)
    if kind == "constant":
        return torch.full((HD,), 0.3125, dtype=BF)
    return (40.0 + 0.4 * torch.randn(HD, generator=g)).to(BF)


@functools.lru_cache(maxsize=None)
def head_prep_inputs(rows, hq, hk, half, seed=5, plant=None):
    """CPU inputs of a layout-0 launch, as test_head_prep_vs_oracle builds them: mixed [rows, (2 hq + 2 hk) 128] bf16 ~ 1.5 N(0, 1),
    rope = cat(sin r, cos r) with r = 6 rand(rows, half), fp32 q / k norms and the bf16 cross-attention norm ~ 0.1 N(0, 1).
    `plant`: one head of that kind in a q, a qx and a k slot (the last of each type), on rows 0, rows // 2 and rows - 1."""
    g = torch.Generator().manual_seed(seed + 1000 * rows + 100 * hq + half)
    n = 2 * hq + 2 * hk
    mixed = (torch.randn(rows, n * HD, generator=g) * 1.5).to(BF)
    r = torch.rand(rows, half, generator=g) * 6.0
    rope = torch.cat([torch.sin(r), torch.cos(r)], dim=-1)
    qn = (0.1 * torch.randn(HD, generator=g), 0.1 * torch.randn(HD, generator=g))
    kn = (0.1 * torch.randn(HD, generator=g), 0.1 * torch.randn(HD, generator=g))
    xn = ((0.1 * torch.randn(HD, generator=g)).to(BF), (0.1 * torch.randn(HD, generator=g)).to(BF))
    if plant is not None:
        m3 = mixed.view(rows, n, HD)
        for row in sorted({0, rows // 2, rows - 1}):
            for slot in (hq - 1, 2 * hq - 1, 2 * hq + hk - 1):
                m3[row, slot] = plant_head(plant, g)
    return dict(mixed=mixed, rope=rope, qn=qn, kn=kn, xn=xn, rows=rows, hq=hq, hk=hk, half=half)


def split_mixed(inp):
    """(q, qx, k, v) views [rows, heads, 128] of the layout-0 row."""
    rows, hq, hk = inp["rows"], inp["hq"], inp["hk"]
    m = inp["mixed"].view(rows, 2 * hq + 2 * hk, HD)
    return m[:, :hq], m[:, hq:2 * hq], m[:, 2 * hq:2 * hq + hk], m[:, 2 * hq + hk:]


def head_prep_reference(inp, q_scale=0.0, one_p=True, eps=EPS):
    """The oracle of part A: q, k, qx, v [rows, heads, 128] bf16, and `q_ln` / `k_ln`, the un-rotated fp32 LayerNorm (x the scale for
    q) rounded once — what the channels behind the rotary width must hold."""
    cfg = MB.MagiLayerConfig(apply_layernorm_1p=one_p, layernorm_epsilon=eps)
    half = inp["half"]
    sin, cos = inp["rope"][:, :half], inp["rope"][:, half:]
    s = torch.tensor(q_scale if q_scale > 0 else 1.0, dtype=torch.float32)
    q, qx, k, v = split_mixed(inp)
    out = {}
    for name, t, n, sc in (("q", q, inp["qn"], s), ("k", k, inp["kn"], None)):
        ln = MB.fused_layer_norm(t.float(), n[0], n[1], cfg)                        # fp32 module on an fp32 tensor
        rot = MB.apply_rotary(ln[None], cos, sin)[0]                                # [1, rows, heads, 128], stays fp32
        assert rot.dtype == torch.float32
        out[name] = (rot * sc if sc is not None else rot).to(BF)
        out[name + "_ln"] = (ln * sc if sc is not None else ln).to(BF)
    out["qx"] = MB.fused_layer_norm(qx, inp["xn"][0], inp["xn"][1], cfg)            # bf16 module on a bf16 tensor
    out["v"] = v.contiguous()
    return out


def kx_reference(kvx, xn, hk, one_p=True, eps=EPS):
    """Layout 1, [rows, hk x (kx | v)]: (kx [rows, hk, 128] through the bf16 LayerNorm, v a copy)."""
    cfg = MB.MagiLayerConfig(apply_layernorm_1p=one_p, layernorm_epsilon=eps)
    kv3 = kvx.view(kvx.shape[0], hk, 2 * HD)
    return MB.fused_layer_norm(kv3[..., :HD], xn[0], xn[1], cfg), kv3[..., HD:].contiguous()


# ---- head prep: the kernel's arithmetic restated in fp32 torch, one step at a time, and its single-step departures ---------------------
MUTATIONS = ("round_before_scale", "w1p_bf16_qk", "w1p_fp32_qx", "drop_1p", "rope_row_off", "omit_scale", "eps_1e-5")


def head_prep_restatement(inp, q_scale=0.0, one_p=True, eps=EPS, mutation=None):
    """magi_head_prep_kernel in fp32 torch ops: per-head two-pass statistics (mean, then the squared deviations), `w + 1` in the
    parameter dtype (fp32 for q / k, bf16 for qx), separately rounded rotary products (elementwise fp32 ops), the scale before the
    ONE rounding.  `mutation` departs from it in one step (MUTATIONS)."""
    assert mutation is None or mutation in MUTATIONS
    half = inp["half"]
    rope = inp["rope"].roll(1, 0) if mutation == "rope_row_off" else inp["rope"]
    sin, cos = rope[:, None, :half], rope[:, None, half:]
    if mutation == "eps_1e-5":
        eps = 1e-5
    if mutation == "drop_1p":
        one_p = False
    s = torch.tensor(1.0 if (q_scale <= 0 or mutation == "omit_scale") else q_scale, dtype=torch.float32)

    def normalised(t):
        x = t.float()
        mean = x.sum(-1, keepdim=True) * (1.0 / HD)
        d = x - mean
        var = (d * d).sum(-1, keepdim=True) * (1.0 / HD)
        return d * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))

    def qk(t, n):
        w, b = n
        if one_p:
            w = (w.to(BF) + 1).float() if mutation == "w1p_bf16_qk" else w + 1
        y = normalised(t) * w + b
        x1, x2 = y[..., :half], y[..., half:2 * half]
        return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos, y[..., 2 * half:]], dim=-1)

    q, qx, k, v = split_mixed(inp)
    rq = qk(q, inp["qn"])
    out = {"q": (rq.to(BF).float() * s).to(BF) if mutation == "round_before_scale" else (rq * s).to(BF),
           "k": qk(k, inp["kn"]).to(BF), "v": v.contiguous()}
    xw, xb = inp["xn"]
    if one_p:
        xw = xw.float() + 1 if mutation == "w1p_fp32_qx" else (xw + 1).float()
    else:
        xw = xw.float()
    out["qx"] = (normalised(qx) * xw + xb.float()).to(BF)
    return out


# ---- quantisers ---------------------------------------------------------------------------------------------------------------------------
def all_finite_bf16():
    """Every finite bf16 bit pattern (both zeros, the subnormals, up to +-3.39e38), 65 280 values as one [120, 544] tensor."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF).reshape(120, 544).clone()


def cycling_divisor(K):
    return torch.tensor(DIVISORS, dtype=torch.float32)[torch.arange(K) % len(DIVISORS)].contiguous()


def quant_reference(x, divisor, fmt, via_bf16):
    """ifx_quant_static on the CPU, uint8 bytes: q = cast(clamp(x / divisor, +-QMAX)), the clamped quotient rounded to bf16 first when
    `via_bf16` (e4m3: `MB.div_clamp_to`, the reference's routine); int8 rounds half to even."""
    d = divisor.float().reshape(-1)
    if fmt == "e4m3":
        if via_bf16:
            return MB.div_clamp_to(x, d).view(torch.uint8)
        return torch.clamp(x.float() / d, -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    v = torch.clamp(x.float() / d, -127.0, 127.0)
    if via_bf16:
        v = v.bfloat16().float()
    return torch.round(v).to(torch.int8).view(torch.uint8)


def per_tensor_reference(x, fmt):
    """(bytes, scale) of ifx_quant_per_tensor: s = max|x| / QMAX in fp32 (1 for an all-zero tensor), q = cast(clamp(x / s))."""
    amax = x.float().abs().max()
    s = amax / QMAX[fmt] if float(amax) > 0 else torch.tensor(1.0)
    return quant_reference(x, s.reshape(1), fmt, False), s


def quant_rows(rows, K, seed=0):
    """bf16 rows ~ 2 N(0, 1) and a divisor vector around 0.03-0.045: quotients ~ N(0, 55), a few beyond +-127, rarely beyond +-448."""
    g = torch.Generator().manual_seed(7 * K + rows + seed)
    x = (2.0 * torch.randn(rows, K, generator=g)).to(BF)
    x[0, 0], x[-1, -1] = 40.0, -40.0                                               # both formats saturate at both corners
    return x, (0.03 * (1 + 0.5 * torch.rand(K, generator=g))).contiguous()


# ---- windows (the pattern of tests/test_hip_row_kernels.py): NaN around an input, a finite sentinel around an output -------------------
def window(t, col0, fill, extra=40, device="cuda"):
    """(buffer, view): `t` as the column window [col0, col0 + cols) of a buffer `cols + col0 + extra` wide filled with `fill`."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + col0 + extra), fill, dtype=t.dtype, device=device)
    view = buf[:, col0:col0 + cols]
    view.copy_(t)
    return buf, view


def margins_intact(buf, col0, cols, fill):
    return bool((buf[:, :col0] == fill).all()) and bool((buf[:, col0 + cols:] == fill).all())


# ---- activations over every bf16 value ----------------------------------------------------------------------------------------------------
ACT_BANDS = (0.0, 2.0 ** -20, 2.0 ** -3, 16.0, 128.0, math.inf)


def act_reference(x, mode):
    return F.silu(x) if mode == "silu" else torch.tanh(x.float()).to(BF)


def act_bands(x):
    """Masks that cut the inputs by sign and magnitude.  `assert_bf16_parity` takes its ULP at max(|ref|, floor x tensor RMS); over all
    finite bf16 values the RMS is ~1e37 and the bar is empty below 1e35, so the same bar is applied to each band on its own as well."""
    a = x.float()
    for neg in (False, True):
        for lo, hi in zip(ACT_BANDS[:-1], ACT_BANDS[1:]):
            m = (a.abs() >= lo) & (a.abs() < hi) & (torch.signbit(a) == neg)
            if bool(m.any()):
                yield f"{'-' if neg else '+'}[{lo:g}, {hi:g})", m

"""GPU: the three kernels of the MAGI ViT-VAE tile decoder (inferix_amd/csrc/ifx_vit.hip), each against its own reference.
  head prep     the operator chain of `Attention.forward` (tests/magi_vit_util.py: torch's bf16 operators on the CPU), through the rule of
                the sister kernel ifx_magi_head_prep: 2 ULP at max(|ref|, tensor RMS), the pair modulus for rotated rows, no element
                exempted.
  attention     fp64 softmax-attention of the same bf16 inputs.  Floor rule: the reference formulation (fp32 softmax, probabilities and
                output rounded to bf16, torch on the CPU) sits `floor` away from fp64 in rel-L2; the kernel must be within
                1.25 x floor + 5e-4.
  unpatch conv  torch's fp32 conv3d on the rearranged tensor, rounded once: <= 1 bf16 ULP on the whole volume, borders included."""
import functools

import pytest
import torch
import torch.nn.functional as F

import magi_vit_util as U
from util import assert_bf16_parity, pair_modulus, rel_l2, ulp_report

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def gpu(t):
    return t.cuda()


# ---------------------------------------------------------------------------------------------------------------------------------
# head prep
def _tables(g, rows):
    ang = torch.rand(rows, 32, generator=g) * 6.2831853
    return ang.sin().to(BF).repeat_interleave(2, -1).contiguous(), ang.cos().to(BF).repeat_interleave(2, -1).contiguous()


def _prep_case(ops, heads, tokens, mode, cls, batch=1, window=False, constant_head=False):
    g = torch.Generator().manual_seed(heads * 1000 + tokens * 10 + cls)
    width = 3 * heads * 64
    qkv = (torch.randn(batch, tokens, width, generator=g) * 1.5 + 0.3 * torch.randn(batch, tokens, 3 * heads, 1, generator=g)
           .expand(-1, -1, -1, 64).reshape(batch, tokens, width)).to(BF)
    if constant_head:
        qkv.view(batch, tokens, 3 * heads, 64)[0, tokens - 1, 1] = 0.7578125          # std = 0: the quotient by eps alone
    norm, rope = mode in ("norm", "both"), mode in ("rope", "both")
    sin = cos = None
    if rope and tokens > cls:
        sin, cos = _tables(g, tokens - cls)
    elif rope:
        sin, cos = torch.zeros(0, 64, dtype=BF), torch.zeros(0, 64, dtype=BF)
    ref = U.head_prep_chain(qkv, heads, cls, norm, sin, cos).reshape(batch * tokens, width)
    if window:
        frame = torch.full((batch * tokens + 2, width + 16), float("nan"), dtype=BF)
        frame[1:-1, 8:8 + width] = qkv.reshape(-1, width)
        dev = gpu(frame)
        buf = dev[1:-1, 8:8 + width]
    else:
        dev = buf = gpu(qkv.reshape(-1, width).clone())
    ops.vit_head_prep(buf, batch=batch, heads=heads, cls_tokens=cls, norm=norm, eps=U.LN_EPS,
                      sin=gpu(sin) if rope else None, cos=gpu(cos) if rope else None)
    got = buf.cpu()
    # the pair modulus is the operand scale of the rotated rows only: q and k of the tokens behind the class token
    scale = torch.zeros_like(ref, dtype=torch.float64).view(batch, tokens, 3, heads * 64)
    if rope:
        scale[:, cls:, :2] = pair_modulus(ref.view(batch, tokens, 3, heads * 64)[:, cls:, :2])
    return got, ref, scale.view_as(ref), dev, qkv


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("mode", ["norm", "rope", "both"])
@pytest.mark.parametrize("tokens", [1, 33, 257])
@pytest.mark.parametrize("heads", [1, 4, 16])
def test_head_prep_against_the_bf16_operator_chain(ops, heads, tokens, mode, cls):
    got, ref, scale, _, qkv = _prep_case(ops, heads, tokens, mode, cls, batch=2 if tokens == 33 else 1)
    assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, scale=scale, what=f"head prep {heads}h {tokens}t {mode} cls{cls}",
                       report=(heads, tokens) == (16, 257))
    if mode == "rope":          # what the rotation does not touch is bit-exact: v, and q / k of the class token
        src = qkv.view(-1, tokens, 3, heads * 64)
        out = got.view(-1, tokens, 3, heads * 64)
        assert torch.equal(out[:, :, 2], src[:, :, 2]) and torch.equal(out[:, :cls], src[:, :cls])


def test_head_prep_strided_window_in_a_nan_frame(ops):
    """A row-strided window: the frame around it stays NaN; v is normalised but not rotated, token 0 is not rotated."""
    heads, tokens = 4, 33
    got, ref, scale, dev, qkv = _prep_case(ops, heads, tokens, "both", 1, batch=2, window=True)
    assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, scale=scale, what="head prep window")
    frame = dev.cpu()
    inside = torch.zeros_like(frame, dtype=torch.bool)
    inside[1:-1, 8:8 + 3 * heads * 64] = True
    assert torch.isnan(frame[~inside].float()).all() and not torch.isnan(frame[inside].float()).any(), "the frame was written"
    normed = U.head_prep_chain(qkv, heads, 1, True).view(2, tokens, 3, heads * 64)
    out = got.view(2, tokens, 3, heads * 64)
    assert_bf16_parity(out[:, :, 2], normed[:, :, 2], max_ulp=2, floor=1.0, what="v: normalised, not rotated")
    assert_bf16_parity(out[:, :1, :2], normed[:, :1, :2], max_ulp=2, floor=1.0, what="class token: not rotated")
    assert not torch.equal(out[:, 1:, :2], normed[:, 1:, :2])


def test_head_prep_constant_head(ops):
    """A head whose 64 channels are equal: std = 0, the quotient is by eps alone, and the result is that of the CPU chain (zeros)."""
    got, ref, scale, _, _ = _prep_case(ops, 4, 33, "norm", 1, constant_head=True)
    row = got.view(33, 12, 64)[32, 1]
    assert torch.equal(row, ref.view(33, 12, 64)[32, 1]) and float(row.abs().max()) == 0.0
    assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, what="head prep with a constant head")


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
def _attn_refs(q, k, v, rows=None):
    """q / k / v `[B, N, H, 64]` bf16 -> (fp64 attention, the reference formulation in bf16) for the query rows `rows` (default all)."""
    qs = q if rows is None else q[:, rows]
    s64 = torch.einsum("bqhd,bkhd->bhqk", qs.double(), k.double()) / 8.0
    exact = torch.einsum("bhqk,bkhd->bqhd", s64.softmax(-1), v.double())
    s32 = torch.einsum("bqhd,bkhd->bhqk", qs.float(), k.float()) / 8.0
    formulation = torch.einsum("bhqk,bkhd->bqhd", s32.softmax(-1).to(BF).float(), v.float()).to(BF)
    return exact, formulation


def _attn_inputs(tokens, heads, batch, seed=0, heavy=False):
    g = torch.Generator().manual_seed(seed + tokens * 100 + heads * 10 + batch)
    q, k, v = (torch.randn(batch, tokens, heads, 64, generator=g) for _ in range(3))
    if heavy:
        # the largest scores sit in the LAST, ragged key tile: every query leans on one direction that only the keys of the last tile
        # carry (score ~ 16 +- 2.5 against ~ N(0, 1.4) elsewhere), so the running maximum moves at the very end; heavy-tailed values
        u = F.normalize(torch.randn(heads, 64, generator=g), dim=-1)
        q = q + 8.0 * u
        last = (tokens - 1) // 64 * 64
        k[:, last:] = k[:, last:] + 16.0 * u
        v = v * torch.exp(1.5 * torch.randn(batch, tokens, heads, 1, generator=g))
    return q.to(BF), k.to(BF), v.to(BF)


def _check_attention(got, exact, formulation, what, report=False):
    floor = rel_l2(formulation, exact)
    err = rel_l2(got, exact)
    bound = 1.25 * floor + 5e-4
    line = f"{what}: kernel vs fp64 {err:.3e}, formulation vs fp64 (floor) {floor:.3e}, bound {bound:.3e}; vs formulation: {ulp_report(got, formulation)}"
    if report:
        print(line)
    assert torch.isfinite(got.float()).all() and err <= bound, line


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("heads", [1, 16])
@pytest.mark.parametrize("tokens", [1, 33, 64, 65, 130, 257])
def test_attention_against_fp64(ops, tokens, heads, batch):
    """q / k / v as the column blocks of one qkv buffer with a strided output window in a NaN frame, and as three separate tensors with a
    dense output: the same bits, within the floor rule of fp64.  batch 2: the second tile's rows must not see the first's keys."""
    q, k, v = _attn_inputs(tokens, heads, batch)
    exact, formulation = _attn_refs(q, k, v)
    D = heads * 64
    rows = batch * tokens
    sep = ops.vit_attention(gpu(q.reshape(rows, D)), gpu(k.reshape(rows, D)), gpu(v.reshape(rows, D)), batch=batch, heads=heads).cpu()
    qkv = gpu(torch.cat((q.reshape(rows, D), k.reshape(rows, D), v.reshape(rows, D)), dim=1))
    frame = torch.full((rows + 2, D + 16), float("nan"), dtype=BF, device="cuda")
    ops.vit_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], batch=batch, heads=heads, out=frame[1:-1, 8:8 + D])
    frame = frame.cpu()
    packed = frame[1:-1, 8:8 + D]
    assert torch.equal(packed, sep), "column blocks of one buffer and separate tensors"
    inside = torch.zeros_like(frame, dtype=torch.bool)
    inside[1:-1, 8:8 + D] = True
    assert torch.isnan(frame[~inside].float()).all(), "the frame around the output window was written"
    _check_attention(sep.view(batch, tokens, heads, 64), exact, formulation, f"attention {tokens}t {heads}h b{batch}",
                     report=(tokens, heads, batch) == (257, 16, 2))


def test_attention_real_tile(ops):
    """4097 tokens x 16 heads, the published tile; compared on the first and last query tiles and one in the middle."""
    tokens, heads = 4097, 16
    q, k, v = _attn_inputs(tokens, heads, 1, seed=7)
    rows = torch.cat((torch.arange(0, 64), torch.arange(2017, 2081), torch.arange(3968, 4097)))
    exact, formulation = _attn_refs(q, k, v, rows)
    got = ops.vit_attention(gpu(q.reshape(tokens, -1)), gpu(k.reshape(tokens, -1)), gpu(v.reshape(tokens, -1)), batch=1, heads=heads)
    got = got.cpu().view(1, tokens, heads, 64)
    assert torch.isfinite(got.float()).all()
    _check_attention(got[:, rows], exact, formulation, "attention 4097t 16h", report=True)


@pytest.mark.parametrize("tokens", [130, 65])
def test_attention_heavy_tail_in_the_last_ragged_tile(ops, tokens):
    q, k, v = _attn_inputs(tokens, 4, 2, seed=3, heavy=True)
    exact, formulation = _attn_refs(q, k, v)
    last = (tokens - 1) // 64 * 64
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / 8.0
    assert bool((s.argmax(-1) >= last).all()), "the case must put every row's maximum into the last key tile"
    rows = 2 * tokens
    got = ops.vit_attention(gpu(q.reshape(rows, -1)), gpu(k.reshape(rows, -1)), gpu(v.reshape(rows, -1)), batch=2, heads=4).cpu()
    _check_attention(got.view(2, tokens, 4, 64), exact, formulation, f"heavy tail {tokens}t", report=True)


def test_attention_padding_keys_have_no_effect_and_launches_are_deterministic(ops):
    """65 tokens: the memory behind row 64 (the rest of the second key tile) is zero, then NaN: the same bits.  Two launches: the same
    bits."""
    tokens, heads, D = 65, 4, 256
    q, k, v = _attn_inputs(tokens, heads, 1, seed=5)
    outs = []
    for fill in (0.0, float("nan"), float("nan")):
        bufs = []
        for t in (q, k, v):
            b = torch.full((128, D), fill, dtype=BF)
            b[:tokens] = t.reshape(tokens, D)
            bufs.append(gpu(b))
        o = torch.full((128, D), 7.0, dtype=BF, device="cuda")
        ops.vit_attention(bufs[0][:tokens], bufs[1][:tokens], bufs[2][:tokens], batch=1, heads=heads, out=o[:tokens])
        o = o.cpu()
        assert bool((o[tokens:] == 7.0).all()), "rows past the end were stored"
        outs.append(o[:tokens])
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]), "padding keys changed the result"
    assert torch.equal(outs[1], outs[2]), "two launches differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# unpatch + 3 x 3 x 3 convolution
@functools.lru_cache(maxsize=None)
def _conv_weights():
    g = torch.Generator().manual_seed(99)
    return (torch.randn(3, 4, 3, 3, 3, generator=g) * 108 ** -0.5).to(BF), (0.1 * torch.randn(3, generator=g)).to(BF)


@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("latent", [(1, 1, 1), (2, 3, 5), (4, 8, 8)])
def test_unpatch_conv_against_fp32_conv3d(ops, latent, cls):
    batch, (pt, ph, pw) = 2, (4, 8, 8)
    lt, lh, lw = latent
    n = lt * lh * lw
    g = torch.Generator().manual_seed(n + cls)
    rows = torch.randn(batch, n + cls, pt * ph * pw * 4, generator=g).to(BF)
    w, b = _conv_weights()
    vol = rows[:, cls:].float().reshape(batch, lt, lh, lw, pt, ph, pw, 4).permute(0, 7, 1, 4, 2, 5, 3, 6)
    vol = vol.reshape(batch, 4, lt * pt, lh * ph, lw * pw)
    ref = F.conv3d(vol, w.float(), b.float(), stride=1, padding=1).to(BF)
    got = ops.vit_unpatch_conv(gpu(rows.reshape(batch * (n + cls), -1)), gpu(w), gpu(b), batch=batch, cls_tokens=cls, latent=latent,
                               patch=(pt, ph, pw)).cpu()
    assert got.shape == ref.shape == (batch, 3, lt * pt, lh * ph, lw * pw)
    assert_bf16_parity(got, ref, max_ulp=1, floor=1.0, what=f"unpatch conv {latent} cls{cls}", report=latent == (4, 8, 8))
    # every face, edge and corner pixel of the volume, on its own
    border = torch.zeros(ref.shape[2:], dtype=torch.bool)
    border[[0, -1]] = True
    border[:, [0, -1]] = True
    border[:, :, [0, -1]] = True
    assert_bf16_parity(got[:, :, border], ref[:, :, border], max_ulp=1, floor=1.0, what=f"unpatch conv border {latent}")

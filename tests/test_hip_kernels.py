"""GPU parity tests: every C-ABI kernel of libinferix_hip.so against the CPU oracle on identical
seeded inputs (teacher-forced per op).  Run on the MI355X box: pytest -m gpu."""
import math

import pytest
import torch

import wan_oracle as O
from util import assert_bf16_parity, pair_modulus, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def gpu(t):
    return t.cuda()


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


@pytest.mark.parametrize("rows,dim,fs", [(72, 256, 24), (4680, 1536, 1560), (77, 1536, 77), (9, 2048, 3), (9, 1160, 3)])
def test_layernorm_modes(ops, rows, dim, fs):
    g = torch.Generator().manual_seed(rows + dim)
    x = rnd(g, 1, rows, dim, scale=2.0)
    groups = (rows + fs - 1) // fs
    # plain
    got = ops.layernorm(gpu(x), 1e-6)
    assert_bf16_parity(got, O.layer_norm(x, 1e-6), what="LN plain")
    # affine (norm3)
    w, b = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF), (0.1 * torch.randn(dim, generator=g)).to(BF)
    got = ops.layernorm(gpu(x), 1e-6, gamma=gpu(w), beta=gpu(b))
    assert_bf16_parity(got, O.layer_norm(x, 1e-6, w, b), what="LN affine")
    # AdaLN modulate with per-frame rows of (modulation + e0)
    if rows % fs == 0:
        mod = rnd(g, groups, 6, dim, scale=0.5)
        e = mod.unsqueeze(0).chunk(6, dim=2)            # [1, groups, 1, dim] each
        for shift_slot, scale_slot in ((0, 1), (3, 4)):
            ref = O.modulate(O.layer_norm(x, 1e-6), e[scale_slot], e[shift_slot], groups)
            got = ops.layernorm(gpu(x), 1e-6, mod=gpu(mod), shift_slot=shift_slot, scale_slot=scale_slot,
                                rows_per_group=fs)
            assert_bf16_parity(got, ref, max_ulp=2, floor=1.0, what=f"AdaLN slots {shift_slot},{scale_slot}")


def test_layernorm_golden(ops):
    from fixture_io import golden
    fx = golden("ops.npz")
    xn = fx["norm_x"]
    assert_bf16_parity(ops.layernorm(gpu(xn), 1e-6), fx["ln_out"], what="golden LN")
    assert_bf16_parity(ops.layernorm(gpu(xn), 1e-6, gamma=gpu(fx["rms_w"]), beta=gpu(fx["ln_b"])),
                       fx["ln_affine_out"], what="golden LN affine")
    mod = (fx["mod"].unsqueeze(1) + fx["e0"]).flatten(0, 1)          # [B*F, 6, dim]
    got = ops.layernorm(gpu(xn), 1e-6, mod=gpu(mod.contiguous()), shift_slot=0, scale_slot=1, rows_per_group=16)
    assert_bf16_parity(got, fx["modulate_out"], floor=1.0, what="golden modulate")
    assert_bf16_parity(ops.rmsnorm(gpu(xn), gpu(fx["rms_w"]), 1e-6), fx["rms_out"], what="golden RMSNorm")


@pytest.mark.parametrize("rows,dim", [(72, 256), (4680, 1536), (513, 1536), (9, 1160)])
def test_rmsnorm(ops, rows, dim):
    g = torch.Generator().manual_seed(rows)
    x = rnd(g, rows, dim, scale=3.0)
    w = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    assert_bf16_parity(ops.rmsnorm(gpu(x), gpu(w), 1e-6), O.rms_norm(x, w, 1e-6), max_ulp=2, what="RMSNorm")


# head_dim 96 does not divide 512: the general per-chunk rotation (axis pairs 16 / 16 / 16); 64 takes the shared (cos, sin) pairs at
# another head size (12 / 10 / 10).  The ids of the head_dim 128 cases are the ones they had before head_dim became a parameter.
@pytest.mark.parametrize("heads,grid,start_frame,ws,rank,hd", [
    (2, (3, 4, 6), 0, 1, 0, 128), (2, (3, 4, 6), 5, 1, 0, 128), (12, (3, 4, 6), 2, 1, 0, 128),
    (2, (3, 4, 6), 3, 2, 1, 128), (2, (3, 4, 6), 3, 4, 3, 128), (12, (3, 30, 52), 18, 1, 0, 128),
    (2, (3, 4, 6), 5, 1, 0, 96), (2, (3, 4, 6), 3, 2, 1, 96), (2, (3, 4, 6), 5, 1, 0, 64), (2, (3, 4, 6), 3, 2, 1, 64)],
    ids=["2-grid0-0-1-0", "2-grid1-5-1-0", "12-grid2-2-1-0", "2-grid3-3-2-1", "2-grid4-3-4-3", "12-grid5-18-1-0",
         "hd96-ws1", "hd96-ws2-rank1", "hd64-ws1", "hd64-ws2-rank1"])
def test_rmsnorm_rope_kv_append(ops, heads, grid, start_frame, ws, rank, hd):
    dim = heads * hd
    f, h, w = grid
    hw_local = h * w // ws
    rows = f * hw_local
    g = torch.Generator().manual_seed(heads * 100 + start_frame + ws)
    qkv = rnd(g, rows, 3 * dim, scale=2.0)
    wq = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    wk = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF)
    freqs = O.rope_freqs(hd)
    q, k, v = qkv.split(dim, dim=1)
    rq = O.causal_rope_apply(O.rms_norm(q, wq, 1e-6).view(1, rows, heads, hd), grid, freqs, start_frame, ws, rank)
    rk = O.causal_rope_apply(O.rms_norm(k, wk, 1e-6).view(1, rows, heads, hd), grid, freqs, start_frame, ws, rank)
    cap = rows * 2 + 5
    local_start = rows // 2 + 3
    kc = torch.zeros(cap, heads, hd, dtype=BF, device="cuda")
    vc = torch.zeros(cap, heads, hd, dtype=BF, device="cuda")
    rope = ops.RopeGridSpec(torch.view_as_real(freqs).contiguous().cuda(), start_frame, h, w, rank * hw_local, hw_local)
    qo = ops.rmsnorm_rope_kv_append(gpu(qkv), gpu(wq), gpu(wk), 1e-6, rope, ops.KvCacheView(kc, vc), local_start, dim)
    assert_bf16_parity(qo.view(rows, heads, hd), rq[0], max_ulp=2, floor=1.0, scale=pair_modulus(rq[0]), what="roped q")
    assert_bf16_parity(kc[local_start:local_start + rows], rk[0], max_ulp=2, floor=1.0, scale=pair_modulus(rk[0]), what="cache K")
    assert torch.equal(vc[local_start:local_start + rows].cpu(), v.reshape(rows, heads, hd)), "cache V must be bit-exact"
    # slots outside [local_start, local_start+rows) untouched
    assert float(kc[:local_start].abs().max()) == 0 and float(kc[local_start + rows:].abs().max()) == 0
    # no-rope / no-append mode (cross-attention query)
    qn = ops.rmsnorm_rope_kv_append(gpu(qkv), gpu(wq), None, 1e-6, None, None, 0, dim)
    assert_bf16_parity(qn, O.rms_norm(q, wq, 1e-6), max_ulp=2, what="rmsnorm-only q")   # two bf16 roundings chained


@pytest.mark.parametrize("ws,rank", [(1, 0), (2, 1)])
@pytest.mark.parametrize("heads", [2, 12])
def test_kv_push_equals_append(ops, heads, ws, rank):
    """ifx_rmsnorm_rope_kv_push (K / V of this rank's rows stored into every destination cache, at the slots of the single-device token
    order) against ifx_rmsnorm_rope_kv_append on the same rows: K and V bit for bit in both destinations, every other slot untouched."""
    hd, (f, h, w) = 128, (3, 4, 6)
    dim = heads * hd
    frame_tokens = h * w
    hw_local = frame_tokens // ws
    hw_offset = rank * hw_local
    rows = f * hw_local
    g = torch.Generator().manual_seed(heads * 10 + ws)
    qkv = gpu(rnd(g, rows, 3 * dim, scale=2.0))
    wq = gpu((1 + 0.1 * torch.randn(dim, generator=g)).to(BF))
    wk = gpu((1 + 0.1 * torch.randn(dim, generator=g)).to(BF))
    rope = ops.RopeGridSpec(torch.view_as_real(O.rope_freqs(hd)).contiguous().cuda(), 2, h, w, hw_offset, hw_local)
    local_start = 7
    cap = local_start + f * frame_tokens + 5
    kc, vc = (torch.zeros(cap, heads, hd, dtype=BF, device="cuda") for _ in range(2))
    ops.rmsnorm_rope_kv_append(qkv, wq, wk, 1e-6, rope, ops.KvCacheView(kc, vc), local_start, dim)
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


def test_rope_golden(ops):
    """RoPE against the reference-generated vectors (identity RMSNorm: weight 1 and pre-normalised rows
    cannot be arranged, so compare through the oracle-equal path on the same inputs instead)."""
    from fixture_io import golden
    fx = golden("ops.npz")
    x = fx["rope_x"]                      # [2, 72, 2, 128]
    freqs = O.rope_freqs(128)
    dim = 256
    ones = torch.ones(dim, dtype=BF)
    for sf in (0, 5):
        for b in range(2):
            xb = x[b].reshape(72, dim)
            qkv = torch.cat([xb, xb, xb], dim=1)
            ref = O.causal_rope_apply(O.rms_norm(xb, ones, 1e-6).view(1, 72, 2, 128), (3, 4, 6), freqs, sf)
            rope = ops.RopeGridSpec(torch.view_as_real(freqs).contiguous().cuda(), sf, 4, 6)
            qo = ops.rmsnorm_rope_kv_append(gpu(qkv), gpu(ones), None, 1e-6, rope, None, 0, dim)
            assert_bf16_parity(qo.view(72, 2, 128), ref[0], floor=1.0, what="rope golden path")


def _attn_case(ops, rows, heads, kv_len, cap=None, seed=0, page=None, splits=None, prescaled=False):
    g = torch.Generator().manual_seed(seed + rows + kv_len)
    hd = 128
    q = rnd(g, rows, heads, hd)
    q_call, scale = q, 0.0
    if prescaled:
        # the exponent fast path: q carries softmax_scale * log2(e) (rounded to bf16 ONCE, as the norm / RoPE kernel does with
        # ifx_rope_grid.q_scale) and the call says scale = ln 2; the fp64 reference below is evaluated on exactly that q
        q_scale, scale = ops.attn_q_prescale(hd)
        q_call = (q.float() * q_scale).to(BF)
    k = rnd(g, kv_len, heads, hd)
    v = rnd(g, kv_len, heads, hd)
    cap = cap or kv_len
    if page is None:
        kc = torch.full((cap, heads, hd), float("nan"), dtype=BF)     # garbage beyond kv_len must not leak
        vc = torch.full((cap, heads, hd), float("nan"), dtype=BF)
        kc[:kv_len], vc[:kv_len] = k, v
        view = ops.KvCacheView(gpu(kc), gpu(vc))
    else:
        ps = page
        npg = (cap + ps - 1) // ps
        perm = torch.randperm(npg, generator=g)
        kc = torch.zeros(npg * ps, heads, hd, dtype=BF)
        vc = torch.zeros(npg * ps, heads, hd, dtype=BF)
        t = torch.arange(kv_len)
        slot = perm[t // ps] * ps + t % ps
        kc[slot], vc[slot] = k, v
        view = ops.KvCacheView(gpu(kc), gpu(vc), gpu(perm.to(torch.int32)), ps)
    out, lse = ops.attention(gpu(q_call), view, kv_len, scale=scale, return_lse=True, splits=splits)
    torch.cuda.synchronize()
    q64 = q_call.double() * (scale * math.sqrt(hd)) if prescaled else q
    ref64, lse64 = O.attention_with_lse(q64[None], k[None], v[None])
    ref_bf = O.attention(q[None], k[None], v[None])            # the reference's CPU path (SDPA bf16)
    err_gpu = (out.cpu().double() - ref64[0]).abs().max().item()
    err_ref = (ref_bf[0].double() - ref64[0]).abs().max().item()
    # stated tolerance: the HIP kernel is as close to exact (fp64) attention as the reference's own
    # bf16 SDPA path is (x2 slack + 1 bf16 ulp of the output scale), and within 1e-3 rel-L2 of it... 
    assert err_gpu <= 2 * err_ref + 4e-3, (err_gpu, err_ref)
    assert rel_l2(out.cpu(), ref64[0]) <= max(1.5 * rel_l2(ref_bf[0], ref64[0]), 3e-3)
    assert (lse.cpu().double() - lse64[0]).abs().max().item() < 2e-3
    return out


@pytest.mark.parametrize("rows,heads,kv_len", [(40, 2, 100), (128, 2, 64), (129, 2, 65), (72, 2, 216),
                                                (32, 12, 1), (200, 12, 513), (72, 2, 63)])
def test_attention_small(ops, rows, heads, kv_len):
    _attn_case(ops, rows, heads, kv_len, cap=kv_len + 7)


def test_attention_golden(ops):
    from fixture_io import golden
    fx = golden("ops.npz")
    q, k, v = fx["attn_q"][0], fx["attn_k"][0], fx["attn_v"][0]
    out = ops.attention(gpu(q), ops.KvCacheView(gpu(k), gpu(v)), k.shape[0])
    ref64 = O.attention(q[None], k[None], v[None], impl="math")[0]
    e_gpu = (out.cpu().double() - ref64).abs().max().item()
    e_ref = (fx["attn_out"][0].double() - ref64).abs().max().item()
    assert e_gpu <= 2 * e_ref + 4e-3
    # two bf16-P flash-attention implementations differ by the rounding of P (2^-9 rel per probability):
    # ~1.5e-3 rel-L2 on random data, the noise floor of the reference's own SDPA/FA path vs exact attention
    assert_bf16_parity(out, fx["attn_out"][0], max_ulp=4, max_mismatch_frac=0.5, rel=3e-3, floor=1.0, what="attention vs reference SDPA")


def test_attention_paged(ops):
    _attn_case(ops, 72, 2, 200, cap=240, page=24)
    _attn_case(ops, 130, 12, 1000, cap=1560, page=120)


@pytest.mark.parametrize("variant", [7, 6, 2])
def test_attention_page_geometries_on_the_pingpong_kernels(ops, variant):
    """The wave-uniform page translation of the ping-pong kernels (PAGED = 1: one scalar table lookup per page, boundary pieces patched
    per lane) against the SAME launch over a contiguous cache, bit for bit: page sizes that divide the 4-key request pieces (1560,
    64), that make pieces straddle pages (130, 7, 3), a two-segment view with an odd split, ragged key ranges, key ranges that start
    inside a page (partial launches), split launches — unused cache slots hold NaN.  One- and two-row pages take the per-lane form on
    the plain two-group schedule (PAGED = 2): compared against exact attention at the usual bound."""
    g = torch.Generator().manual_seed(77)
    rows, heads, hd = 600, 12, 128
    L = 4680 + 1560 + 37
    q, k, v = rnd(g, rows, heads, hd), rnd(g, L, heads, hd), rnd(g, L, heads, hd)
    qs, scale = ops.attn_q_prescale(hd)
    qg = gpu((q.float() * qs).to(BF))
    kg, vg = gpu(k), gpu(v)

    def paged_view(ps):
        npg = (L + ps - 1) // ps + 2
        perm = torch.randperm(npg, generator=g)
        kc = torch.full((npg * ps, heads, hd), float("nan"), dtype=BF)
        vc = torch.full((npg * ps, heads, hd), float("nan"), dtype=BF)
        t = torch.arange(L)
        slot = perm[t // ps] * ps + t % ps
        kc[slot], vc[slot] = k, v
        return ops.KvCacheView(gpu(kc), gpu(vc), gpu(perm.to(torch.int32)), ps)

    def segment_view(split, delta):
        kc = torch.full((L + delta, heads, hd), float("nan"), dtype=BF)
        vc = torch.full((L + delta, heads, hd), float("nan"), dtype=BF)
        kc[:split], vc[:split] = k[:split], v[:split]
        kc[split + delta:], vc[split + delta:] = k[split:], v[split:]
        return ops.KvCacheView(gpu(kc), gpu(vc), None, 1, split, delta)

    def run(view, kv_len, kv_start, splits):
        if kv_start == 0:
            return ops.attention(qg, view, kv_len, scale=scale, splits=splits)
        s = splits or 2
        ws = ops.attention_workspace(qg, s)
        u = ops.attention_partial(qg, view, kv_len, kv_start, s, ws, 0, s, scale=scale)
        out = torch.empty_like(qg)
        ops.attention_merge(ws, s, u, out)
        return out

    cases = [(L, 0, 1), (L, 0, 3), (4680 + 1560, 0, 1), (L, 4680, 2), (L - 5, 1563, 2)]
    with ops.option_scope("attn_variant", variant):
        plain = ops.KvCacheView(kg, vg)
        refs = [run(plain, *c).clone() for c in cases]
        views = [("page 1560", paged_view(1560)), ("page 64", paged_view(64)), ("page 130", paged_view(130)), ("page 7", paged_view(7)),
                 ("page 3", paged_view(3)), ("segments 4681 + 11", segment_view(4681, 11)), ("segments 6000 + 4", segment_view(6000, 4))]
        for name, view in views:
            for c, ref in zip(cases, refs):
                out = run(view, *c)
                assert torch.equal(out, ref), (name, c, float((out.float() - ref.float()).abs().max()))
        ref64 = O.attention((qg[:64].cpu().double() * (scale * math.sqrt(hd)))[None], k[None], v[None], impl="math")[0]
        for ps in (1, 2):
            view = paged_view(ps)
            for c, ref in zip(cases, refs):
                out = run(view, *c)
                assert torch.isfinite(out.float()).all()
                assert rel_l2(out.cpu(), ref.cpu()) < 5e-3, (ps, c)
                if c == cases[0]:
                    assert (out[:64].cpu().double() - ref64).abs().max().item() < 1.5e-2, ps


@pytest.mark.parametrize("rows,heads,kv_len,splits,page", [
    (72, 2, 1000, 2, None), (129, 2, 1025, 3, None), (300, 12, 2048, 7, None), (40, 2, 130, 5, None),
    (130, 12, 1000, 4, 120), (72, 2, 200, 2, 24), (585, 12, 4680, None, None)])
def test_attention_split_kv(ops, rows, heads, kv_len, splits, page):
    """Split-KV launch (sequence-parallel shard shapes): chunks run as independent workgroups, fp32 partials are
    merged before the single bf16 rounding -> same bound vs exact attention as the unsplit kernel."""
    _attn_case(ops, rows, heads, kv_len, cap=(kv_len + 119) // 120 * 120 if page else kv_len + 5, page=page, splits=splits)


def test_attention_split_plan_and_workspace_errors(ops):
    import ctypes as C
    from inferix_amd import _hip
    lib = _hip.load()
    need = C.c_int64(-1)
    assert lib.ifx_attn_split_plan(4680, 12, 0, 32760, C.byref(need)) == 1 and need.value == 0
    s = lib.ifx_attn_split_plan(585, 12, 0, 32760, C.byref(need))
    assert 2 <= s <= 32 and need.value == s * 585 * 12 * 129 * 4
    assert lib.ifx_attn_split_plan(585, 12, 0, 512, C.byref(need)) == 1          # too few keys to split
    g = torch.Generator().manual_seed(0)
    q, k = gpu(rnd(g, 64, 2, 128)), gpu(rnd(g, 256, 2, 128))
    ws = torch.empty(16, dtype=torch.float32, device="cuda")
    ks = ops.KvCacheView(k, k).struct()
    rc = lib.ifx_attn_fwd_paged_split(q.data_ptr(), torch.empty_like(q).data_ptr(), None, C.byref(ks), 64, 2, 0, 256, 0.0,
                                      2, ws.data_ptr(), 64, None)
    assert rc != 0 and b"workspace" in lib.ifx_last_error()
    rc = lib.ifx_attn_fwd_paged_split(q.data_ptr(), torch.empty_like(q).data_ptr(), None, C.byref(ks), 64, 2, 0, 256, 0.0,
                                      0, None, 0, None)
    assert rc != 0


def test_attention_partial_launches_share_one_merge(ops):
    """Sequence-parallel form: prefix and new-block keys attended in separate launches that write fp32 partials into one
    workspace, merged once — equals the single launch over all keys."""
    g = torch.Generator().manual_seed(41)
    rows, heads, L, cut = 585, 12, 4680 + 1560 * 3, 4680
    q, k, v = rnd(g, rows, heads, 128), rnd(g, L, heads, 128), rnd(g, L, heads, 128)
    qg, view = gpu(q), ops.KvCacheView(gpu(k), gpu(v))
    full, lse = ops.attention(qg, view, L, return_lse=True, splits=1)
    s1, s2 = ops.attention_split_plan(rows, heads, cut), ops.attention_split_plan(rows, heads, L - cut)
    cap = s1 + s2
    ws = ops.attention_workspace(qg, cap)
    u1 = ops.attention_partial(qg, view, cut, 0, s1, ws, 0, cap)
    u2 = ops.attention_partial(qg, view, L, cut, s2, ws, u1, cap)
    assert 1 <= u1 <= s1 and 1 <= u2 <= s2
    out = torch.empty_like(qg)
    l2 = torch.empty(heads, rows, dtype=torch.float32, device="cuda")
    ops.attention_merge(ws, cap, u1 + u2, out, l2)
    # two groupings of the same keys differ by the bf16 rounding noise of P itself (diffuse softmax, |o| ~ 0.02)
    assert rel_l2(out.cpu(), full.cpu()) < 5e-3 and (l2 - lse).abs().max().item() < 1e-3
    ref64 = O.attention(q[:64][None], k[None], v[None], impl="math")[0]
    assert (out[:64].cpu().double() - ref64).abs().max().item() < 1.5e-2
    from inferix_amd import _hip
    with pytest.raises(_hip.HipKernelError):
        ops.attention_partial(qg, view, L, cut, s2, ws, cap, cap)            # slots beyond the workspace


def test_attention_480p_block_shapes(ops):
    """Real tile geometry: 4680 queries x 12 heads over 1 and 2 cached blocks (CPU fp64 reference on a
    row subset keeps this in seconds)."""
    g = torch.Generator().manual_seed(1)
    rows, heads, hd = 4680, 12, 128
    for kv_len in (4680, 9360):
        q = rnd(g, rows, heads, hd)
        k = rnd(g, kv_len, heads, hd)
        v = rnd(g, kv_len, heads, hd)
        out = ops.attention(gpu(q), ops.KvCacheView(gpu(k), gpu(v)), kv_len)
        sel = torch.cat([torch.arange(0, 64), torch.arange(2300, 2364), torch.arange(4616, 4680)])
        ref64 = O.attention(q[sel][None], k[None], v[None], impl="math")[0]
        ref_bf = O.attention(q[sel][None], k[None], v[None])[0]
        e_gpu = (out[sel.cuda()].cpu().double() - ref64).abs().max().item()
        e_ref = (ref_bf.double() - ref64).abs().max().item()
        r_gpu, r_ref = rel_l2(out[sel.cuda()].cpu().double(), ref64), rel_l2(ref_bf, ref64)
        # same rule as the long-prefix tests below: 1.25 x the reference's own distance from exact attention (+ 5e-4 on the rel-L2,
        # + one bf16 step of the largest output on the max)
        assert r_gpu <= 1.25 * r_ref + 5e-4, (kv_len, r_gpu, r_ref)
        assert e_gpu <= 1.25 * e_ref + float(ref64.abs().max()) * 2.0 ** -8, (kv_len, e_gpu, e_ref)


@pytest.mark.parametrize("kv_len", [14040, 23400, 32760])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_480p_long_prefixes_vs_fp64_oracle(ops, kv_len, paged, prescaled):
    """The prefix lengths of blocks 2 / 4 / 6 of the BASELINE clip (where 70 % of the attention time is): 4680 queries x 12 heads
    over 14040 / 23400 / 32760 cached keys, default schedule, contiguous and through a page table (pages of one frame, shuffled).
    192 query rows (the first, a middle and the last ragged tile) against the CPU fp64 oracle, with the reference's own bf16 SDPA
    measured on the same rows as the yardstick: rel-L2 within 1.25 x the reference's own distance from exact attention + 5e-4 (the block /
    rollout rule), max error within 1.25 x the reference's + one bf16 step of the largest output.
    `prescaled`: the form the model uses — q multiplied by scale * log2(e) before its rounding to bf16, the call with scale = ln 2 (the
    exponent fast path); the fp64 reference is evaluated on that q."""
    g = torch.Generator().manual_seed(kv_len + int(paged))
    rows, heads, hd, fsz = 4680, 12, 128, 1560
    q, k, v = rnd(g, rows, heads, hd), rnd(g, kv_len, heads, hd), rnd(g, kv_len, heads, hd)
    q_call, scale, q64 = q, 0.0, q
    if prescaled:
        q_scale, scale = ops.attn_q_prescale(hd)
        q_call = (q.float() * q_scale).to(BF)
        q64 = q_call.double() * (scale * math.sqrt(hd))
    if paged:
        pages = kv_len // fsz
        perm = torch.randperm(pages, generator=g)
        kp, vp = torch.empty_like(k), torch.empty_like(v)
        kp.view(pages, fsz, heads, hd)[perm] = k.view(pages, fsz, heads, hd)     # logical page i lives in physical page perm[i]
        vp.view(pages, fsz, heads, hd)[perm] = v.view(pages, fsz, heads, hd)
        view = ops.KvCacheView(gpu(kp), gpu(vp), perm.to(torch.int32).cuda(), fsz)
    else:
        view = ops.KvCacheView(gpu(k), gpu(v))
    out, lse = ops.attention(gpu(q_call), view, kv_len, scale=scale, return_lse=True)
    sel = torch.cat([torch.arange(0, 64), torch.arange(2300, 2364), torch.arange(4616, 4680)])
    ref64, lse64 = O.attention_with_lse(q64[sel][None], k[None], v[None])
    ref_bf = O.attention(q[sel][None], k[None], v[None])[0]
    got = out[sel.cuda()].cpu().double()
    e_gpu, e_ref = (got - ref64[0]).abs().max().item(), (ref_bf.double() - ref64[0]).abs().max().item()
    r_gpu, r_ref = rel_l2(got, ref64[0]), rel_l2(ref_bf, ref64[0])
    print(f"L={kv_len} paged={paged} prescaled={prescaled}: max|err| hip {e_gpu:.3e} / reference bf16 SDPA {e_ref:.3e}; rel-L2 hip {r_gpu:.3e} / reference {r_ref:.3e}")
    # the block / rollout rule (1.25 x the reference's own distance from exact attention + 5e-4) on the rel-L2; the max over 295 k
    # elements moves by one bf16 step of the largest outputs between two correct kernels (measured 3.0e-4 vs 2.3e-4 on one launch)
    ulp_top = float(ref64[0].abs().max()) * 2.0 ** -8
    assert r_gpu <= 1.25 * r_ref + 5e-4, (kv_len, r_gpu, r_ref)
    assert e_gpu <= 1.25 * e_ref + ulp_top, (kv_len, e_gpu, e_ref, ulp_top)
    assert (lse[:, sel.cuda()].cpu().double() - lse64[0]).abs().max().item() < 2e-3


@pytest.mark.parametrize("kv_len", [32400, 75600])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_720p_block_at_size_vs_fp64_oracle(ops, kv_len, paged, prescaled):
    """BASELINE config 3 at its REAL size (round-3 verdict: the 720p test ran tiny channels only): a CausVid 720p block is 3 latent
    frames x 3600 tokens = 10800 query rows x 12 heads, over the 32400-key prefix of block 2 and the full 75600-key cache of a
    21-latent segment — the launches whose tile height the rounds-aware choice decides (256-row x 3 rounds against 128-row x 2,
    DESIGN §5).  Default (auto) schedule, contiguous and through a page table with pages of one frame (3600 tokens, shuffled).
    192 query rows (first, middle and last tile) against the CPU fp64 oracle with the reference's bf16 SDPA on the same rows as the
    yardstick: the 1.25 x floor + 5e-4 rule of the 480p test above; LSE to 2e-3.  `prescaled` = the model's exponent form."""
    g = torch.Generator().manual_seed(kv_len + int(paged))
    rows, heads, hd, fsz = 10800, 12, 128, 3600
    q, k, v = rnd(g, rows, heads, hd), rnd(g, kv_len, heads, hd), rnd(g, kv_len, heads, hd)
    q_call, scale, q64 = q, 0.0, q
    if prescaled:
        q_scale, scale = ops.attn_q_prescale(hd)
        q_call = (q.float() * q_scale).to(BF)
        q64 = q_call.double() * (scale * math.sqrt(hd))
    if paged:
        pages = kv_len // fsz
        perm = torch.randperm(pages, generator=g)
        kp, vp = torch.empty_like(k), torch.empty_like(v)
        kp.view(pages, fsz, heads, hd)[perm] = k.view(pages, fsz, heads, hd)     # logical page i lives in physical page perm[i]
        vp.view(pages, fsz, heads, hd)[perm] = v.view(pages, fsz, heads, hd)
        view = ops.KvCacheView(gpu(kp), gpu(vp), perm.to(torch.int32).cuda(), fsz)
    else:
        view = ops.KvCacheView(gpu(k), gpu(v))
    out, lse = ops.attention(gpu(q_call), view, kv_len, scale=scale, return_lse=True)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    sel = torch.cat([torch.arange(0, 64), torch.arange(5300, 5364), torch.arange(10736, 10800)])
    ref64, lse64 = O.attention_with_lse(q64[sel][None], k[None], v[None])
    ref_bf = O.attention(q[sel][None], k[None], v[None])[0]
    got = out[sel.cuda()].cpu().double()
    e_gpu, e_ref = (got - ref64[0]).abs().max().item(), (ref_bf.double() - ref64[0]).abs().max().item()
    r_gpu, r_ref = rel_l2(got, ref64[0]), rel_l2(ref_bf, ref64[0])
    print(f"720p L={kv_len} paged={paged} prescaled={prescaled}: max|err| hip {e_gpu:.3e} / reference bf16 SDPA {e_ref:.3e}; rel-L2 hip {r_gpu:.3e} / reference {r_ref:.3e}")
    # the block / rollout rule (1.25 x the reference's own distance from exact attention + 5e-4) on the rel-L2; the max over 295 k
    # elements moves by one bf16 step of the largest outputs between two correct kernels (measured 3.0e-4 vs 2.3e-4 on one launch)
    ulp_top = float(ref64[0].abs().max()) * 2.0 ** -8
    assert r_gpu <= 1.25 * r_ref + 5e-4, (kv_len, r_gpu, r_ref)
    assert e_gpu <= 1.25 * e_ref + ulp_top, (kv_len, e_gpu, e_ref, ulp_top)
    assert (lse[:, sel.cuda()].cpu().double() - lse64[0]).abs().max().item() < 2e-3
    if prescaled or paged:
        return
    # size-independent properties of the same launch (tests/test_hip_full_size_properties.py does this at the 480p size):
    vf = gpu(v).float()
    vmin, vmax = vf[:kv_len].amin(0), vf[:kv_len].amax(0)
    o = out.float()
    assert (o >= vmin[None] - 1e-2).all() and (o <= vmax[None] + 1e-2).all(), "not a convex combination of the value rows"
    half = (kv_len // 2 // 64) * 64 + 17                                  # an unaligned cut
    o1, l1 = ops.attention(gpu(q), view, half, return_lse=True, splits=1)
    o2, l2 = ops.attention(gpu(q), view, kv_len, return_lse=True, splits=1, kv_start=half)
    ops.lse_merge(o1, l1, o2, l2)
    assert rel_l2(o1.cpu(), out.cpu()) < 4e-3 and (l1 - lse).abs().max() < 1e-3, "split-KV identity"
    sp, lsp = ops.attention(gpu(q), view, kv_len, return_lse=True, splits=3)
    assert rel_l2(sp.cpu(), out.cpu()) < 3e-3 and (lsp - lse).abs().max() < 1e-3
    assert torch.equal(ops.attention(gpu(q), view, kv_len), out), "the launch is deterministic"


@pytest.mark.parametrize("distinct,total", [(40, 512), (63, 512), (64, 512), (1, 512), (200, 1024), (511, 512)])
def test_attention_dedup_equals_attention_over_the_repeated_keys(ops, distinct, total):
    """ifx_attn_fwd_dedup (cross-attention over a zero-padded prompt): `distinct` keys followed by ONE key of multiplicity
    total - distinct equals plain attention over the `total` keys in which that row is repeated — against the fp64 oracle and
    against the plain kernel on the explicit keys."""
    g = torch.Generator().manual_seed(distinct + total)
    rows, heads, hd = 4680 if total == 512 else 300, 12, 128
    q = rnd(g, rows, heads, hd)
    k = rnd(g, total, heads, hd)
    v = rnd(g, total, heads, hd)
    k[distinct:] = k[distinct]
    v[distinct:] = v[distinct]
    view = ops.KvCacheView(gpu(k), gpu(v))
    got = ops.attention_dedup(gpu(q), view, distinct + 1, total - distinct)
    plain = ops.attention(gpu(q), view, total)
    sel = torch.arange(0, rows, max(rows // 96, 1))[:96]
    ref64 = O.attention(q[sel][None], k[None], v[None], impl="math")[0]
    e_d, e_p = rel_l2(got[sel.cuda()].cpu(), ref64), rel_l2(plain[sel.cuda()].cpu(), ref64)
    assert e_d <= 1.25 * e_p + 5e-4, (e_d, e_p)          # as close to exact attention as the plain kernel
    # two evaluations with bf16 probabilities: the repeated key's weight is rounded once here and `multiplicity` times there
    assert rel_l2(got.cpu(), plain.cpu()) < 6e-3
    if distinct == total - 1:                              # multiplicity 1: the same launch as the plain kernel
        assert torch.equal(got, plain)


def test_attention_softmax_spike(ops):
    """Online-softmax rescale path: one key dominates late in the sequence (guide §5.4 rule 26)."""
    g = torch.Generator().manual_seed(3)
    rows, heads, kv_len, hd = 64, 2, 640, 128
    q = rnd(g, rows, heads, hd)
    k = rnd(g, kv_len, heads, hd)
    v = rnd(g, kv_len, heads, hd)
    k[500] = (q[5] * 4).to(BF)                 # huge score for query 5 at tile 7
    k[10] = (q[40] * 6).to(BF)
    out = ops.attention(gpu(q), ops.KvCacheView(gpu(k), gpu(v)), kv_len)
    ref64 = O.attention(q[None], k[None], v[None], impl="math")[0]
    assert (out.cpu().double() - ref64).abs().max().item() < 3e-2
    assert rel_l2(out.cpu(), ref64) < 5e-3


def test_lse_merge_split_kv_equals_full(ops):
    g = torch.Generator().manual_seed(4)
    rows, heads, kv_len, hd = 100, 2, 300, 128
    q, k, v = rnd(g, rows, heads, hd), rnd(g, kv_len, heads, hd), rnd(g, kv_len, heads, hd)
    full = ops.attention(gpu(q), ops.KvCacheView(gpu(k), gpu(v)), kv_len)
    o1, l1 = ops.attention(gpu(q), ops.KvCacheView(gpu(k[:130].contiguous()), gpu(v[:130].contiguous())), 130, return_lse=True)
    o2, l2 = ops.attention(gpu(q), ops.KvCacheView(gpu(k[130:].contiguous()), gpu(v[130:].contiguous())), 170, return_lse=True)
    ops.lse_merge(o1, l1, o2, l2)
    assert rel_l2(o1.cpu(), full.cpu()) < 4e-3
    _, lse64 = O.attention_with_lse(q[None], k[None], v[None])
    assert (l1.cpu().double() - lse64[0]).abs().max().item() < 2e-3


@pytest.mark.parametrize("M,N,K", [(72, 256, 256), (77, 64, 64), (4680, 1536, 1536), (300, 640, 256),
                                   (130, 256, 640), (4680, 64, 1536)])
def test_gemm_bias(ops, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
    got = ops.linear(gpu(x), gpu(w), gpu(b))
    assert_bf16_parity(got, torch.nn.functional.linear(x, w, b), what=f"linear {M}x{N}x{K}")
    got = ops.linear(gpu(x), gpu(w), None)
    assert_bf16_parity(got, torch.nn.functional.linear(x, w), what="linear no bias")


def test_gemm_epilogues(ops):
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(9)
    M, N, K, fs = 144, 256, 640, 48
    x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
    res = rnd(g, M, N)
    mod = rnd(g, M // fs, 6, N, scale=0.5)
    y = torch.nn.functional.linear(x, w, b)
    got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GELU_TANH)
    assert_bf16_parity(got, torch.nn.functional.gelu(y, approximate="tanh"), floor=1.0, what="gelu epilogue")
    got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_RESIDUAL, residual=gpu(res))
    assert_bf16_parity(got, res + y, floor=1.0, what="residual epilogue")
    for slot in (2, 5):
        gate = mod[:, slot].unsqueeze(0).unsqueeze(2)           # [1, F, 1, N]
        ref = O.gated_residual(res[None], y[None], gate, M // fs)[0]
        got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GATE_RES, residual=gpu(res), mod=gpu(mod),
                         gate_slot=slot, rows_per_group=fs)
        assert_bf16_parity(got, ref, floor=1.0, what=f"gate+residual epilogue slot {slot}")


def test_gemm_ffn_real_shapes(ops):
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(10)
    M, d, f = 1560, 1536, 8960
    x, w1, b1 = rnd(g, M, d), rnd(g, f, d, scale=d ** -0.5), rnd(g, f, scale=0.1)
    w2, b2 = rnd(g, d, f, scale=f ** -0.5), rnd(g, d, scale=0.1)
    u = ops.linear(gpu(x), gpu(w1), gpu(b1), epilogue=_hip.IFX_EPI_GELU_TANH)
    u_ref = torch.nn.functional.gelu(torch.nn.functional.linear(x, w1, b1), approximate="tanh")
    assert_bf16_parity(u, u_ref, max_ulp=2, floor=1.0, what="ffn.0+gelu 1536->8960")
    y = ops.linear(gpu(u_ref), gpu(w2), gpu(b2))
    assert_bf16_parity(y, torch.nn.functional.linear(u_ref, w2, b2), what="ffn.2 8960->1536")


_GEMM_CASES = [(v, M, N, K) for v in range(1, 12) for M, N, K in [(585, 1536, 1536), (300, 640, 256), (77, 64, 64), (1170, 4608, 1536)]]
# 12-14 split K between the wave groups of a workgroup: K/64 has to divide by the groups (4, 2, 2)
_GEMM_CASES += [(v, M, N, K) for v in (15, 16, 17) for M, N, K in [(585, 1536, 1536), (300, 640, 256), (77, 64, 64)]]
_GEMM_CASES += [(v, M, N, K) for v in (12, 13, 14) for M, N, K in [(585, 1536, 1536), (300, 640, 256), (77, 64, 512), (585, 1536, 8960)]]
# 18 = four-wave 256x256 on the LDS-DMA ring, 19 = the register-staged software-pipelined four-wave tile (ifx_gemm_w4.hip): one K step
# (K = 64), odd step counts, ragged edges in both dimensions, a tile count that is not a multiple of the XCD count
_GEMM_CASES += [(v, M, N, K) for v in (18, 19) for M, N, K in [(585, 1536, 1536), (300, 640, 64), (77, 64, 192), (1170, 4608, 1536),
                                                                (2000, 2312, 3072)]]


# the 256x192 tile: 96-column wave tiles (a 12-chunk epilogue transpose); ragged M and N edges, N not a multiple of 192
_GEMM_CASES += [(21, M, N, K) for M, N, K in [(585, 1536, 1536), (300, 640, 64), (77, 64, 192), (1170, 4608, 1536), (2000, 2312, 3072),
                                              (4680, 4608, 1536)]]


# 22 / 23 / 24 = the persistent ping-pong tiles (256 / 192 / 128 tokens x 256 channels, ifx_gemm_pp.hip), 25 = 22 without the K split:
# one K step, odd step counts, ragged token edges, N a multiple of 64 but not of 256, fewer tiles than XCDs, several tiles per workgroup,
# and the split shape (N <= 2048, K >= 4096: variant 22 splits through the workspace hip_ops.linear hands over, 25 does not)
_GEMM_CASES += [(v, M, N, K) for v in (22, 23, 24, 25) for M, N, K in [(585, 1536, 1536), (700, 640, 64), (600, 64, 192),
                                                                       (1170, 4608, 1536), (2000, 2304, 3072), (4680, 1536, 8960),
                                                                       (9000, 8960, 128)]]


@pytest.mark.parametrize("variant,M,N,K", _GEMM_CASES)
def test_gemm_every_tile_variant(ops, variant, M, N, K):
    """Each GEMM kernel (register-staged 128x128, LDS-DMA 256x128 / 128x128 / 64x64) on shard shapes with ragged
    M and N edges, all four epilogues; the auto choice is covered by the other tests."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(M + N + variant)
    fs = (M + 2) // 3
    x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
    res, mod = rnd(g, M, N), rnd(g, 3, 6, N, scale=0.5)
    y = torch.nn.functional.linear(x, w, b)
    ops.set_option("gemm_variant", variant)
    try:
        assert_bf16_parity(ops.linear(gpu(x), gpu(w), gpu(b)), y, what=f"variant {variant} bias")
        got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GELU_TANH)
        assert_bf16_parity(got, torch.nn.functional.gelu(y, approximate="tanh"), max_ulp=2, floor=1.0,
                           what=f"variant {variant} gelu")   # bf16(gelu(bf16(y))): two chained roundings
        got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_RESIDUAL, residual=gpu(res))
        assert_bf16_parity(got, res + y, max_ulp=2, floor=1.0, what=f"variant {variant} residual")
        gate = torch.repeat_interleave(mod[:, 2], fs, dim=0)[:M]
        got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GATE_RES, residual=gpu(res), mod=gpu(mod),
                         gate_slot=2, rows_per_group=fs)
        assert_bf16_parity(got, res + (y * gate).to(BF), max_ulp=2, floor=1.0, what=f"variant {variant} gate+residual")
    finally:
        ops.set_option("gemm_variant", 0)


def test_gemm_four_wave_tile_auto_choice_and_split_k(ops):
    """The long-K shapes the auto choice hands to the four-wave tile (MAGI-4.5B fc1 of one rank) agree with the eight-wave tile on
    the same inputs; the split-K form (variant 20, two workgroups per tile through ifx_gemm_bf16_ws) equals the unsplit tile to
    fp32 summation order, is deterministic run to run, and leaves its arrival counters zeroed for the next launch."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(77)
    M, N, K = 6075, 12288, 3072
    x, w = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5))
    auto = ops.linear(x, w, None, epilogue=_hip.IFX_EPI_GELU_ERF)
    ops.set_option("gemm_variant", 5)
    try:
        ref = ops.linear(x, w, None, epilogue=_hip.IFX_EPI_GELU_ERF)
    finally:
        ops.set_option("gemm_variant", 0)
    assert torch.equal(auto, ref), "same MFMA summation order: the two tiles must agree bit for bit"
    M, N, K = 4680, 1536, 8960
    x, w, b, res = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1)), gpu(rnd(g, M, N))
    mod = gpu(rnd(g, 3, 6, N, scale=0.5))
    kw = dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=5, rows_per_group=1560)
    base = ops.linear(x, w, b, **kw)
    ops.set_option("gemm_variant", 20)
    try:
        outs = [ops.linear(x, w, b, **kw) for _ in range(5)]
        assert _hip.load().ifx_gemm_workspace_bytes(M, N, K) > 0
    finally:
        ops.set_option("gemm_variant", 0)
    assert all(torch.equal(o, outs[0]) for o in outs), "split-K result must not depend on which workgroup finishes last"
    # two K halves summed once in fp32 instead of one running sum: a flipped bf16 rounding of y moves bf16(res + bf16(y * gate))
    assert_bf16_parity(outs[0], base, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what="split-K vs single pass")


def test_gemm_ping_pong_split_k_is_deterministic_and_row_invariant(ops):
    """Round 3: the auto choice gives launches of >= 2048 rows to the persistent ping-pong tiles, and splits K over two workgroups per
    tile where N <= 2048 and K >= 4096 (the FFN down-projection) — a rule on (N, K) ONLY.  So: the library asks for a workspace for that
    shape under auto, the result is the same run to run (first half + second half, whoever finishes last), agrees with the unsplit
    tile (variant 25) to fp32 summation order, leaves the flags zero, and a ROW's bits do not depend on how many rows the launch
    has (4680 rows alone == the first 4680 of 9360) — for the split shape and for an unsplit one."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(78)
    lib = _hip.load()
    ops.set_option("gemm_small_split", 0)            # the default; a sequence-parallel attach in this process may have turned it on
    # small launches as well (round-2 verdict: the text-embedding linear, 1536 x 4096, split at one 512-token prompt and not at two)
    for M, N, K in ((512, 1536, 4096), (585, 1536, 8960), (585, 1536, 1536), (300, 4608, 1536)):
        x, w, b = gpu(rnd(g, 2 * M + 2048, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
        one, more = ops.linear(x[:M], w, b), ops.linear(x, w, b)
        assert torch.equal(one, more[:M]), f"{M} x {N} x {K}: a row's bits changed with the number of rows in the launch"
    for (N, K, kw_name) in ((1536, 8960, "gate"), (4608, 1536, "bias")):
        M = 4680
        x, w, b = gpu(rnd(g, 2 * M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
        res, mod = gpu(rnd(g, 2 * M, N)), gpu(rnd(g, 6, 6, N, scale=0.5))
        kw = dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res[:M], mod=mod, gate_slot=5, rows_per_group=1560) if kw_name == "gate" else {}
        kw2 = dict(kw, residual=res) if kw else {}
        assert (lib.ifx_gemm_workspace_bytes(M, N, K) > 0) == (N == 1536)
        outs = [ops.linear(x[:M], w, b, **kw) for _ in range(4)]
        assert all(torch.equal(o, outs[0]) for o in outs)
        both = ops.linear(x, w, b, **kw2)
        assert torch.equal(both[:M], outs[0]), f"N={N} K={K}: a row's bits changed with the number of rows in the launch"
        if N == 1536:
            # 7020 rows (nine 480p frames / a 720p partial block): the split runs on the 192-token tile there (fewer rounds), on the
            # 256-token tile at 4680 and 9360 rows — the tile height must not change a bit
            part = ops.linear(x[:7020], w, b, **dict(kw, residual=res[:7020]))
            assert torch.equal(part[:M], outs[0]), "the 192-token split tile gives other bits than the 256-token one"
        ops.set_option("gemm_variant", 25)
        try:
            single = ops.linear(x[:M], w, b, **kw)
        finally:
            ops.set_option("gemm_variant", 0)
        if N == 1536:
            assert_bf16_parity(outs[0], single, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what="ping-pong split-K vs single pass")
        else:
            assert torch.equal(outs[0], single)
    ws = next(iter(ops._GEMM_WS.values()))
    torch.cuda.synchronize()
    assert int(ws[:4096].view(torch.int32).abs().sum().item()) == 0, "per-tile flags must be left zero"


@pytest.mark.parametrize("M", [7020, 10800])
def test_gemm_ffn_down_720p_rows_vs_fp64(ops, M):
    """Round-4 verdict: the 192-token split tile (FFN down at 7020 / 10800 rows) was checked through a chain of bit-equalities only.
    Direct check: y = bf16(res + bf16(bf16(x W^T + b) * gate)) with the accumulation in fp64 on the device (every row, every channel),
    for the gate + residual epilogue the block uses and for the plain bias epilogue.  fp32 MFMA accumulation over K = 8960 against the
    fp64 sum: the bf16 result may flip one rounding in a few elements per thousand — 2 ULP, <= 2 % of the elements."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(80 + M)
    N, K, fs = 1536, 8960, M // 3
    x, w, b = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
    res, mod = gpu(rnd(g, M, N)), gpu(rnd(g, 3, 6, N, scale=0.5))
    acc = torch.empty(M, N, dtype=torch.float64, device="cuda")
    wd = w.double().t().contiguous()
    for r0 in range(0, M, 1080):                       # row slabs keep the fp64 operands small
        acc[r0:r0 + 1080] = x[r0:r0 + 1080].double() @ wd
    y = (acc + b.double()).to(BF)                      # one rounding of the exact sum (double -> bf16 rounds to nearest even directly)
    assert lib_ws(ops, M, N, K) > 0, "auto must ask for the split-K workspace on this shape"
    got = ops.linear(x, w, b)
    assert_bf16_parity(got, y, max_ulp=1, max_mismatch_frac=0.02, floor=0.05, what=f"FFN down {M} rows, bias")
    gate = torch.repeat_interleave(mod[:, 5], fs, dim=0)[:M]
    want = (res.float() + (y.float() * gate.float()).to(BF).float()).to(BF)
    got = ops.linear(x, w, b, epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=5, rows_per_group=fs)
    assert_bf16_parity(got, want, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what=f"FFN down {M} rows, gate + residual")
    again = ops.linear(x, w, b, epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=5, rows_per_group=fs)
    assert torch.equal(got, again)


def lib_ws(ops, M, N, K):
    from inferix_amd import _hip
    ops.set_option("gemm_small_split", 0)
    return int(_hip.load().ifx_gemm_workspace_bytes(M, N, K))


def test_gemm_second_destination_and_append_without_v(ops):
    """Round 5: the q|k|v projection stores its V columns straight into the KV cache rows (ifx_epilogue.y2 / `linear(out2=)`) and
    ifx_rmsnorm_rope_kv_append is told not to copy V (ifx_rope_grid.flags bit 0).  The two-destination launch must give the bits of the
    plain launch column for column (q|k in `out`, v in the cache rows, nothing else of the cache touched), the V-less append the same
    q and K as the full one, and a launch that the ping-pong tiles cannot serve must be refused, not silently drop the columns."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(97)
    d, heads, fsz = 1536, 12, 1560
    for M in (4680, 2496, 640):                       # 640 rows: the launcher forces the 128-token ping-pong tile
        x, w, b = gpu(rnd(g, M, d)), gpu(rnd(g, 3 * d, d, scale=d ** -0.5)), gpu(rnd(g, 3 * d, scale=0.1))
        plain = ops.linear(x, w, b)
        slots, start = M + 2 * fsz, fsz
        kc = torch.full((slots, heads, 128), 7.0, dtype=BF, device="cuda")
        vc = torch.full((slots, heads, 128), 7.0, dtype=BF, device="cuda")
        out = torch.full((M, 3 * d), 3.0, dtype=BF, device="cuda")
        got = ops.linear(x, w, b, out=out, out2=vc.view(slots, d)[start:start + M], split_col=2 * d)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out[:, :2 * d], plain[:, :2 * d]), f"{M} rows: q|k columns differ from the plain launch"
        assert torch.equal(vc.view(slots, d)[start:start + M], plain[:, 2 * d:]), f"{M} rows: V rows in the cache differ"
        assert bool((out[:, 2 * d:] == 3.0).all()), "the V columns of `out` must not be written"
        assert bool((vc[:start] == 7.0).all()) and bool((vc[start + M:] == 7.0).all()), "cache rows outside the block were touched"
        # append: full (copies V from the projection) against V-less (V already in place)
        view_a = ops.KvCacheView(torch.zeros_like(kc), torch.zeros_like(vc))
        rope = ops.RopeGridSpec(torch.view_as_real(O.rope_freqs(128)).contiguous().cuda(), 1, 30, 52)
        wq, wk = gpu(rnd(g, d)), gpu(rnd(g, d))
        q_a = ops.rmsnorm_rope_kv_append(plain, wq, wk, 1e-6, rope, view_a, start, d)
        view_b = ops.KvCacheView(kc, vc)
        q_b = ops.rmsnorm_rope_kv_append(out, wq, wk, 1e-6, rope, view_b, start, d, v_in_place=True)
        assert torch.equal(q_a, q_b) and torch.equal(view_a.k[start:start + M], kc[start:start + M])
        assert torch.equal(view_a.v[start:start + M], vc[start:start + M])
        assert bool((kc[:start] == 7.0).all()) and bool((kc[start + M:] == 7.0).all())
    x, w, b = gpu(rnd(g, 256, d)), gpu(rnd(g, 3 * d, d, scale=d ** -0.5)), gpu(rnd(g, 3 * d, scale=0.1))
    with pytest.raises(_hip.HipKernelError, match="second destination"):       # a residual epilogue cannot carry it
        ops.linear(x, w, b, epilogue=_hip.IFX_EPI_RESIDUAL, residual=gpu(rnd(g, 256, 3 * d)),
                   out2=torch.empty(256, d, dtype=BF, device="cuda"), split_col=2 * d)
    with pytest.raises(_hip.HipKernelError, match="second destination"):       # split_col must be a multiple of 256
        ops.linear(x, w, b, out2=torch.empty(256, d + 64, dtype=BF, device="cuda"), split_col=2 * d - 64)


def test_gemm_ping_pong_multi_part_split(ops):
    """Round 5: K split over 2 / 4 / 8 workgroups per tile on the 128-token ping-pong tile (gemm_variant 27 / 28 / 29): parts 1 .. ks-1 dump
    fp32 tile images and raise their own flags, part 0 adds them in part order.  Against F.linear in fp32 for every epilogue, the same bits
    run to run (whoever finishes last), flags left zero; and the auto choice of a 4-way sequence-parallel rank (gemm_small_split) takes
    the 4-way form for its FFN down-projection — the same bits as variant 28."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(95)
    fs = 390
    for (M, N, K, variants) in ((1170, 1536, 8960, (27, 28)), (585, 1536, 1536, (27, 28, 29)), (300, 512, 1024, (27, 28, 29))):
        x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
        res, mod = rnd(g, M, N), rnd(g, 3, 6, N, scale=0.5)
        y = torch.nn.functional.linear(x.float(), w.float(), b.float()).to(BF)
        gate = torch.repeat_interleave(mod[:, 2], fs, dim=0)[:M]
        for v in variants:
            ops.set_option("gemm_variant", v)
            try:
                assert _hip.load().ifx_gemm_workspace_bytes(M, N, K) > 0
                got = ops.linear(gpu(x), gpu(w), gpu(b))
                assert_bf16_parity(got, y, max_mismatch_frac=0.03, what=f"variant {v} {M}x{N}x{K} bias")
                again = [ops.linear(gpu(x), gpu(w), gpu(b)) for _ in range(3)]
                assert all(torch.equal(a, got) for a in again), f"variant {v}: the result depends on which part finishes last"
                got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GELU_TANH)
                assert_bf16_parity(got, torch.nn.functional.gelu(y, approximate="tanh"), max_ulp=2, floor=1.0, max_mismatch_frac=0.03,
                                   what=f"variant {v} gelu")
                got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_RESIDUAL, residual=gpu(res))
                assert_bf16_parity(got, res + y, max_ulp=2, floor=1.0, max_mismatch_frac=0.03, what=f"variant {v} residual")
                got = ops.linear(gpu(x), gpu(w), gpu(b), epilogue=_hip.IFX_EPI_GATE_RES, residual=gpu(res), mod=gpu(mod), gate_slot=2,
                                 rows_per_group=fs)
                assert_bf16_parity(got, res + (y * gate).to(BF), max_ulp=2, floor=1.0, max_mismatch_frac=0.03, what=f"variant {v} gate+residual")
            finally:
                ops.set_option("gemm_variant", 0)
    torch.cuda.synchronize()
    for ws in ops._GEMM_WS.values():
        assert int(ws[:4096].view(torch.int32).abs().sum().item()) == 0, "per-part flags must be left zero"
    M, N, K = 1170, 1536, 8960
    x, w, b, res = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1)), gpu(rnd(g, M, N))
    ops.set_option("gemm_variant", 28)
    try:
        forced = ops.linear(x, w, b, epilogue=_hip.IFX_EPI_RESIDUAL, residual=res)
    finally:
        ops.set_option("gemm_variant", 0)
    with ops.option_scope("gemm_small_split", 1):
        assert _hip.load().ifx_gemm_workspace_bytes(M, N, K) > 0 and _hip.load().ifx_gemm_workspace_bytes(585, N, K) == 0
        auto = ops.linear(x, w, b, epilogue=_hip.IFX_EPI_RESIDUAL, residual=res)
    assert torch.equal(auto, forced), "a 4-way rank's FFN down-projection must run the 4-way split of the 128-token tile"


def test_split_k_consumer_wait_is_bounded_and_reported(ops):
    """Round-4 verdict item 7 / ADVICE r3: the split-K consumer of the ping-pong GEMM waits for its partner's flag with a BUDGET.  With the
    lab switch `spin_fault` the producers keep their flags down: the launch must still END (within the budget, not hang the GPU), raise
    the device error word (kind 1), `ifx_last_error` / `check_device` must say so and clear it, the flag page must be left zero, and
    the next ordinary launch of the same shape must be bit-identical to the one before the fault."""
    import time
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(91)
    ops.set_option("gemm_small_split", 0)
    M, N, K = 4680, 1536, 8960
    x, w, b = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
    assert _hip.load().ifx_gemm_workspace_bytes(M, N, K) > 0
    good = ops.linear(x, w, b)
    torch.cuda.synchronize()
    assert ops.device_error() == 0
    assert ops.get_option("spin_timeout_ms") == 2000 and ops.get_option("spin_fault") == 0
    ops.set_option("spin_timeout_ms", 25)
    ops.set_option("spin_fault", 1)
    try:
        t0 = time.perf_counter()
        bad = ops.linear(x, w, b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert dt < 5.0, f"the faulted launch took {dt:.2f} s: the wait is not bounded"
        assert dt > 0.02, "the consumers did not wait for their budget"
        code = ops.device_error(clear=False)
        assert code >> 24 == 1, hex(code)
        with pytest.raises(_hip.HipKernelError, match="gave up a wait"):
            ops.check_device("faulted GEMM")
        assert ops.device_error() == 0, "reporting must clear the word"
        assert bad.shape == good.shape
    finally:
        ops.set_option("spin_fault", 0)
        ops.set_option("spin_timeout_ms", 2000)
    ws = ops._gemm_workspace(x.device, 4096)
    assert int(ws[:4096].view(torch.int32).abs().sum().item()) == 0, "per-tile flags must be left zero by the faulted launch"
    again = ops.linear(x, w, b)
    torch.cuda.synchronize()
    assert torch.equal(again, good) and ops.device_error() == 0


def test_gemm_stream_k_variant_is_correct_and_deterministic(ops):
    """gemm_variant 26 (lab only: it lost to the in-workgroup split tiles at the shard sizes it was written for): equal K-step ranges
    over the workgroups, the tile's owner adds the later ranges' partial sums in ascending K order.  Same values as the auto choice up
    to the summation split, bit-identical run to run, flags left zero, every epilogue."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(17)
    for M, N, K, kw_name in ((585, 4608, 1536, "bias"), (585, 1536, 8960, "gate"), (585, 8960, 1536, "gelu"), (1170, 1536, 1536, "res"),
                             (300, 512, 1024, "bias")):
        x, w, b = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
        res, mod = gpu(rnd(g, M, N)), gpu(rnd(g, 6, 6, N, scale=0.5))
        kw = {"bias": {}, "gelu": dict(epilogue=_hip.IFX_EPI_GELU_TANH), "res": dict(epilogue=_hip.IFX_EPI_RESIDUAL, residual=res),
              "gate": dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=5, rows_per_group=195)}[kw_name]
        want = ops.linear(x, w, b, **kw)
        ops.set_option("gemm_variant", 26)
        try:
            outs = [ops.linear(x, w, b, **kw) for _ in range(3)]
        finally:
            ops.set_option("gemm_variant", 0)
        assert all(torch.equal(o, outs[0]) for o in outs), (M, N, K)
        assert_bf16_parity(outs[0], want, max_ulp=2, max_mismatch_frac=0.02, floor=1.0, what=f"stream-K {M}x{N}x{K} {kw_name}")
    torch.cuda.synchronize()
    for ws in ops._GEMM_WS.values():
        assert int(ws[:4096].view(torch.int32).abs().sum().item()) == 0, "per-workgroup flags must be left zero"


def test_gemm_small_split_auto_choice_at_2340_rows(ops):
    """Round 4: under `gemm_small_split` (what a sequence-parallel model's forward scopes on) the narrow-N launches of a 2-way rank —
    2340 rows x 1536 channels, K = 1536 and 8960: 228 tiles of 128 x 128 — take the in-workgroup split tile (variant 14) ahead of the
    ping-pong tiles; without the option the auto choice is untouched.  Same bits as the forced variant, fp64-close, every epilogue."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(2340)
    M, N, fs = 2340, 1536, 780
    try:
        for K in (1536, 8960):
            x, w, b = gpu(rnd(g, M, K)), gpu(rnd(g, N, K, scale=K ** -0.5)), gpu(rnd(g, N, scale=0.1))
            res, mod = gpu(rnd(g, M, N)), gpu(rnd(g, M // fs, 6, N, scale=0.5))
            for kw in ({}, dict(epilogue=_hip.IFX_EPI_RESIDUAL, residual=res),
                       dict(epilogue=_hip.IFX_EPI_GATE_RES, residual=res, mod=mod, gate_slot=2, rows_per_group=fs)):
                ops.set_option("gemm_small_split", 0)
                plain = ops.linear(x, w, b, **kw)
                ops.set_option("gemm_variant", 14)
                forced = ops.linear(x, w, b, **kw)
                ops.set_option("gemm_variant", 0)
                # (K = 8960: the default is the ping-pong tile's two-workgroup K split, first half + second half — the same two halves tile
                #  12 adds, so the bits coincide; K = 1536: single pass against two halves)
                assert torch.equal(plain, forced) == (K == 8960)
                ops.set_option("gemm_small_split", 1)
                auto = ops.linear(x, w, b, **kw)
                assert torch.equal(auto, forced), f"K={K}: the auto choice under gemm_small_split is not tile 12"
                assert_bf16_parity(auto, plain, max_ulp=2, max_mismatch_frac=0.03, floor=1.0, what=f"tile 12 vs default, K={K}")
            y64 = x.cpu().double() @ w.cpu().double().t() + b.cpu().double()
            assert rel_l2(ops.linear(x, w, b).cpu().double(), y64) < 3e-3
    finally:
        ops.set_option("gemm_variant", 0)
        ops.set_option("gemm_small_split", 0)


def test_gemm_split_k_tiles_refuse_indivisible_k(ops):
    """A forced split-K tile on a K it cannot split evenly is an error, not a silently different kernel; the auto choice
    (variant 0) only picks those tiles when K divides."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(3)
    x, w, b = rnd(g, 77, 192), rnd(g, 64, 192), rnd(g, 64)
    ops.set_option("gemm_variant", 12)
    try:
        with pytest.raises(_hip.HipKernelError, match="K-groups"):
            ops.linear(gpu(x), gpu(w), gpu(b))
    finally:
        ops.set_option("gemm_variant", 0)
    assert_bf16_parity(ops.linear(gpu(x), gpu(w), gpu(b)), torch.nn.functional.linear(x, w, b), what="auto tile, K = 192")
    # small launches whose K splits: the auto choice takes the split-K tiles (head linear / text embedding / shard shapes)
    for M, N, K in [(585, 1536, 1536), (585, 1536, 8960), (4680, 64, 1536), (512, 1536, 4096), (2340, 1536, 8960)]:
        x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N, scale=0.1)
        assert_bf16_parity(ops.linear(gpu(x), gpu(w), gpu(b)), torch.nn.functional.linear(x, w, b), what=f"auto {M}x{N}x{K}")


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7])
def test_attention_both_kernels(ops, variant):
    ops.set_option("attn_variant", variant)
    try:
        if variant in (6, 7):                                  # loops unrolled 6 / 4 times over constant LDS slots: every remainder
            for tiles in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13):
                _attn_case(ops, 260, 2, 64 * tiles - 9, cap=64 * tiles)
                _attn_case(ops, 140, 3, 64 * tiles, cap=64 * tiles + 64, page=64)
        _attn_case(ops, 300, 12, 2048, cap=2100)
        _attn_case(ops, 130, 12, 1000, cap=1560, page=120)
        _attn_case(ops, 1000, 2, 700, cap=777)                 # several query tiles, ragged last key tile
        _attn_case(ops, 390, 3, 64, cap=64)                    # a single key tile
        _attn_case(ops, 200, 2, 100, cap=128)                  # two key tiles, ragged (even tile count of the parity-unrolled loop)
        _attn_case(ops, 200, 2, 190, cap=192)                  # three key tiles, ragged (odd tile count)
        _attn_case(ops, 70, 2, 40, cap=64)                     # one ragged tile
        _attn_case(ops, 500, 2, 1111, cap=1200, splits=3)
    finally:
        ops.set_option("attn_variant", 0)


@pytest.mark.parametrize("variant", [0, 6, 7])
def test_attention_prescaled_q_exponent_fast_path(ops, variant):
    """scale * log2(e) == 1: `attn_fwd_pp_kernel<.., 7>` (and `<.., 8>`, the two-per-CU form) applies exp2 straight to the MFMA accumulators (the reference maximum enters as the
    C operand).  Every remainder of the four-times unrolled loop, ragged / paged / split launches, the kernels without the fast path
    (short prefixes, small launches: same call, generic arithmetic), and the redo path of the lazy maximum."""
    ops.set_option("attn_variant", variant)
    try:
        for tiles in (1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13):
            _attn_case(ops, 260, 2, 64 * tiles - 9, cap=64 * tiles, prescaled=True)
            _attn_case(ops, 140, 3, 64 * tiles, cap=64 * tiles + 64, page=64, prescaled=True)
        _attn_case(ops, 300, 12, 2048, cap=2100, prescaled=True)
        _attn_case(ops, 130, 12, 1000, cap=1560, page=120, prescaled=True)
        _attn_case(ops, 1000, 2, 700, cap=777, prescaled=True)
        _attn_case(ops, 70, 2, 40, cap=64, prescaled=True)
        _attn_case(ops, 500, 2, 1111, cap=1200, splits=3, prescaled=True)
        _attn_case(ops, 1200, 12, 4680, prescaled=True)
        # one key dominates late in the sequence: the tile outgrows the reference maximum (redo + rescale + the next tile's scores corrected)
        g = torch.Generator().manual_seed(3)
        rows, heads, kv_len, hd = 300, 2, 900, 128
        q, k, v = rnd(g, rows, heads, hd), rnd(g, kv_len, heads, hd), rnd(g, kv_len, heads, hd)
        k[500] = (q[5] * 4).to(BF)
        k[10] = (q[40] * 6).to(BF)
        k[700] = (q[290] * 5).to(BF)
        q_scale, scale = ops.attn_q_prescale(hd)
        qs = (q.float() * q_scale).to(BF)
        out = ops.attention(gpu(qs), ops.KvCacheView(gpu(k), gpu(v)), kv_len, scale=scale, splits=1)
        ref64, _ = O.attention_with_lse((qs.double() * (scale * math.sqrt(hd)))[None], k[None], v[None])
        assert (out.cpu().double() - ref64[0]).abs().max().item() < 3e-2
        assert rel_l2(out.cpu(), ref64[0]) < 5e-3
    finally:
        ops.set_option("attn_variant", 0)


def test_rope_q_scale_is_one_rounding(ops):
    """ifx_rope_grid.q_scale: q_out == bf16(q_fp32 * q_scale) — checked against the unscaled kernel output, whose bf16 values bracket
    the fp32 q: |q_scaled - bf16(q_out * q_scale)| stays within one bf16 ulp, K and V written to the cache do not change."""
    from inferix_amd.wan import components as C
    g = torch.Generator().manual_seed(11)
    rows, H, hd = 3 * 24, 2, 128
    d = H * hd
    qkv = rnd(g, rows, 3 * d)
    wq, wk = rnd(g, d, scale=0.3) + 1.0, rnd(g, d, scale=0.3) + 1.0
    freqs = C.rope_table(hd).cuda()
    q_scale, _ = ops.attn_q_prescale(hd)
    outs = []
    for qs in (0.0, q_scale):
        kc, vc = torch.zeros(rows, H, hd, dtype=BF, device="cuda"), torch.zeros(rows, H, hd, dtype=BF, device="cuda")
        rope = ops.RopeGridSpec(freqs, 2, 4, 6, q_scale=qs)
        qo = ops.rmsnorm_rope_kv_append(gpu(qkv), gpu(wq), gpu(wk), 1e-6, rope, ops.KvCacheView(kc, vc), 0, d)
        outs.append((qo.cpu(), kc.cpu(), vc.cpu()))
    (q0, k0, v0), (q1, k1, v1) = outs
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    want = q0.float() * q_scale
    ulp = torch.maximum(want.abs(), torch.tensor(1e-30)) * 2.0 ** -7      # one bf16 ulp of the value's binade, generously
    assert ((q1.float() - want).abs() <= ulp).all()


def test_kernels_are_run_to_run_deterministic(ops):
    """Same inputs -> same bits, launch after launch (a v_max3 inline-asm read scheduled right behind the last
    S MFMA once read stale accumulators: still valid softmax, but timing-dependent roundings).  Shapes large enough
    that waves of different workgroups share SIMDs."""
    from inferix_amd import _hip
    g = torch.Generator().manual_seed(21)
    rows, heads, L, dim, ffn = 585, 12, 4680, 1536, 8960
    q, k, v = gpu(rnd(g, rows, heads, 128)), gpu(rnd(g, L, heads, 128)), gpu(rnd(g, L, heads, 128))
    x, w, b = gpu(rnd(g, rows, dim)), gpu(rnd(g, ffn, dim, scale=dim ** -0.5)), gpu(rnd(g, ffn, scale=0.1))
    junk = torch.zeros(2048, 2048, device="cuda")

    def stable(fn, reps=40):
        ref = fn().clone()
        for i in range(reps):
            if i % 3 == 0:
                junk.add_(1.0)
            if not torch.equal(fn(), ref):
                return False
        return True
    try:
        for av in (1, 2, 3, 4, 5, 6, 7):
            ops.set_option("attn_variant", av)
            assert stable(lambda: ops.attention(q, ops.KvCacheView(k, v), L, splits=1)), f"attention variant {av}"
        ops.set_option("attn_variant", 0)
        assert stable(lambda: ops.attention(q, ops.KvCacheView(k, v), L, splits=4)), "split-KV attention"
        for gv in (1, 2, 3, 4, 5, 6, 12, 13, 14, 21):
            ops.set_option("gemm_variant", gv)
            assert stable(lambda: ops.linear(x, w, b, epilogue=_hip.IFX_EPI_GELU_TANH), reps=15), f"gemm variant {gv}"
    finally:
        ops.set_option("attn_variant", 0)
        ops.set_option("gemm_variant", 0)


@pytest.mark.parametrize("paged", [False, True])
def test_kv_scatter_shards(ops, paged):
    """Rank-major gathered K/V rows land in the (frame, rank, hw) token order, bit-exact (integer permutation)."""
    g = torch.Generator().manual_seed(31)
    P, frames, hw_local, heads, hd = 4, 3, 6, 2, 128
    fs, local_start, cap = P * hw_local, 48, 168
    n_local = frames * hw_local
    gathered = rnd(g, P, 2, n_local, heads, hd)
    k0, v0 = rnd(g, cap, heads, hd), rnd(g, cap, heads, hd)
    pt, ps = None, 1
    if paged:
        ps = fs
        pt = torch.randperm(cap // ps, generator=g).to(torch.int32)
    kr, vr = k0.clone(), v0.clone()
    for r in range(P):
        for f in range(frames):
            for i in range(hw_local):
                tok = local_start + f * fs + r * hw_local + i
                slot = int(pt[tok // ps]) * ps + tok % ps if paged else tok
                kr[slot], vr[slot] = gathered[r, 0, f * hw_local + i], gathered[r, 1, f * hw_local + i]
    kg, vg = gpu(k0), gpu(v0)
    ops.kv_scatter_shards(gpu(gathered), P, frames, hw_local, fs, local_start,
                          ops.KvCacheView(kg, vg, gpu(pt) if paged else None, ps))
    assert torch.equal(kg.cpu(), kr) and torch.equal(vg.cpu(), vr)
    from inferix_amd import _hip
    with pytest.raises(_hip.HipKernelError):
        ops.kv_scatter_shards(gpu(gathered), P, frames, hw_local, fs, cap - 10, ops.KvCacheView(kg, vg))


def test_kv_roll(ops):
    g = torch.Generator().manual_seed(12)
    cap, heads, hd = 144, 2, 128
    k, v = rnd(g, cap, heads, hd), rnd(g, cap, heads, hd)
    sink, ev, rolled = 24, 72, 48
    kk, vv = k.clone(), v.clone()
    kk[sink:sink + rolled] = k[sink + ev:sink + ev + rolled]
    vv[sink:sink + rolled] = v[sink + ev:sink + ev + rolled]
    kg, vg = gpu(k), gpu(v)
    ops.kv_roll(ops.KvCacheView(kg, vg), sink, ev, rolled, torch.empty(rolled * heads * hd, dtype=BF, device="cuda"))
    assert torch.equal(kg.cpu(), kk) and torch.equal(vg.cpu(), vv)


def test_errors_are_loud(ops):
    from inferix_amd import _hip
    x = torch.zeros(4, 100, dtype=BF, device="cuda")          # dim % 8 != 0
    with pytest.raises(_hip.HipKernelError):
        ops.layernorm(x, 1e-6)
    with pytest.raises(_hip.HipKernelError):
        ops.layernorm(torch.zeros(4, 128, dtype=BF), 1e-6)    # CPU tensor: refuse, no fallback
    with pytest.raises(_hip.HipKernelError):
        ops.linear(torch.zeros(4, 100, dtype=BF, device="cuda"), torch.zeros(8, 100, dtype=BF, device="cuda"), None)

"""MAGI's 8-bit (e4m3) cache on the GPU (include/inferix_hip_kv8_magi.h): the ranges launch over a two-segment key map against fp64
attention over the dequantised bytes (yardstick: the fp64 emulation that rounds P to e4m3, as tests/test_hip_attn_kv8.py), each range
bit for bit against the single launch on a contiguous copy of its keys, and the head-prep kernel's bytes against an fp32 restatement."""
import math

import pytest
import torch

import magi_rows_util as U
from util import rel_l2

pytestmark = pytest.mark.gpu
BF, F8, HD = torch.bfloat16, torch.float8_e4m3fn, 128
Q_SCALE = HD ** -0.5 * math.log2(math.e)
SLOTS, SEG_BASE, KEYS = 1300, 700, 549          # the scratch segment starts well behind the in-place rows; logical keys [0, 549)
Q_SIZES = (70, 300)                             # a tile with a tail; a range over two row tiles
K_RANGES = [(0, 64), (100, 300), (0, 449), (100, 164), (0, 200), (100, 549)]      # starts 0 / 100 (inside a tile) x lengths 64 / 200 / 449


@pytest.fixture(scope="module")
def ops():
    from inferix_amd import hip_ops
    return hip_ops


def deq(b):
    return b.view(F8).double()


def softmax64(q8, k8, v8, v_scale, group):
    """(fp64 attention over the dequantised bytes, the same with P = exp2(s - max + 7) rounded to e4m3): [rows, heads, 128] each."""
    qd = deq(q8).transpose(0, 1)
    kd = deq(k8).repeat_interleave(group, dim=1).transpose(0, 1)
    vd = (deq(v8) * v_scale.view(1, -1, 1).double()).repeat_interleave(group, dim=1).transpose(0, 1)
    s = qd @ kd.transpose(1, 2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    p8 = (p * 128).float().to(F8).double()
    return ((p @ vd) / l).transpose(0, 1), ((p8 @ vd) / (l * 128)).transpose(0, 1)


def e4m3(x):
    return x.float().clamp(-448, 448).to(F8).view(torch.uint8)


def build(hq, hk, n_ranges, seg_split, seed):
    """q8 with 3 unread rows between the query ranges, the logical keys, and the cache planes: NaN bytes in every slot no key maps to."""
    g = torch.Generator().manual_seed(seed)
    q_ranges, row = [], 0
    for i in range(n_ranges):
        q_ranges.append((row, row + Q_SIZES[i % 2]))
        row += Q_SIZES[i % 2] + 3
    k_ranges = [K_RANGES[i % len(K_RANGES)] for i in range(n_ranges)]
    q8 = e4m3(torch.randn(row, hq, HD, generator=g) * 3 * Q_SCALE)
    v_scale = torch.tensor([2.0, 0.5])[:hk]
    k8, v8 = e4m3(torch.randn(KEYS, hk, HD, generator=g)), e4m3(torch.randn(KEYS, hk, HD, generator=g) / v_scale.view(1, hk, 1))
    j = torch.arange(KEYS)
    slot = torch.where(j >= seg_split, SEG_BASE + j - seg_split, j) if seg_split else j
    kc, vc = (torch.full((SLOTS, hk, HD), 0x7F, dtype=torch.uint8) for _ in range(2))
    kc[slot], vc[slot] = k8, v8
    return q8, k8, v8, v_scale, kc, vc, q_ranges, k_ranges


#        hq hk ranges seg_split strided
CASES = [(2, 2, 1, 0, False), (6, 2, 3, 128, False), (6, 2, 8, 150, False), (2, 2, 3, 150, True), (6, 2, 8, 0, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_ranges_vs_fp64(ops, case):
    hq, hk, n, seg_split, strided = case
    q8, k8, v8, v_scale, kc, vc, q_ranges, k_ranges = build(hq, hk, n, seg_split, 7 + n)
    rows, d = q8.shape[0], hq * HD
    view = ops.MagiKv8View(kc.cuda(), vc.cuda(), v_scale.cuda(), seg_split, SEG_BASE if seg_split else 0)
    qbuf = torch.full((rows, d + (48 if strided else 0)), 0x7F, dtype=torch.uint8, device="cuda")
    obuf = torch.full((rows, d + (24 if strided else 0)), 7.0, dtype=BF, device="cuda")
    qg, og = (qbuf[:, 16:16 + d], obuf[:, 8:8 + d]) if strided else (qbuf, obuf)
    qg.copy_(q8.view(rows, d))
    ops.attention_kv8_ranges(qg, view, q_ranges, k_ranges, og, hq)
    got = obuf.cpu()
    if strided:
        assert bool((got[:, :8] == 7.0).all()) and bool((got[:, 8 + d:] == 7.0).all()), "columns outside the output window were written"
        got = got[:, 8:8 + d]
    written = torch.zeros(rows, dtype=torch.bool)
    for (qs, qe), (ks, ke) in zip(q_ranges, k_ranges):
        written[qs:qe] = True
        out64, emu64 = softmax64(q8[qs:qe], k8[ks:ke], v8[ks:ke], v_scale, hq // hk)
        rel, rel_emu = rel_l2(got[qs:qe].view(-1, hq, HD), out64), rel_l2(emu64, out64)
        print(f"kv8 ranges {case} q [{qs}, {qe}) k [{ks}, {ke}): rel-L2 {rel:.3e}, emulation {rel_emu:.3e}, bound {1.25 * rel_emu + 1e-3:.3e}")
        assert rel <= 1.25 * rel_emu + 1e-3          # (NaN compares false)
    assert bool((got[~written] == 7.0).all()), "rows outside every query range were written"


@pytest.mark.parametrize("hq,seg_split", [(2, 0), (6, 128)])
def test_range_isolation(ops, hq, seg_split):
    """Each range of a 3-range launch against ifx_attn_fwd_kv8 on that range alone over a contiguous copy of its keys, bit for bit.
    The ranges are those whose tile list the cut at seg_split leaves as it is: [0, 200) is cut after two whole tiles, [128, 549) and
    [200, 300) lie in the scratch segment (the latter starting inside it); a cut inside a tile moves the tile boundaries and with them
    the grid P is rounded on, which the tolerance test above covers."""
    hk = 2
    q8, k8, v8, v_scale, kc, vc, q_ranges, _ = build(hq, hk, 3, seg_split, 11)
    k_ranges = [(0, 200), (128, KEYS), (200, 300)]
    view = ops.MagiKv8View(kc.cuda(), vc.cuda(), v_scale.cuda(), seg_split, SEG_BASE if seg_split else 0)
    rows, d = q8.shape[0], hq * HD
    out = torch.zeros(rows, d, dtype=BF, device="cuda")
    ops.attention_kv8_ranges(q8.view(rows, d).cuda(), view, q_ranges, k_ranges, out, hq)
    for (qs, qe), (ks, ke) in zip(q_ranges, k_ranges):
        pad = torch.full((3, hk, HD), 0x7F, dtype=torch.uint8)
        flat = ops.Kv8CacheView(torch.cat([k8[ks:ke], pad]).cuda(), torch.cat([v8[ks:ke], pad]).cuda(), v_scale.cuda())
        alone = ops.attention_kv8(q8[qs:qe].cuda(), flat, ke - ks)
        assert torch.equal(out[qs:qe].view(-1, hq, HD), alone), f"range q [{qs}, {qe}) k [{ks}, {ke}) differs from its own launch"


def _restate(inp, q_scale, v_scale, flip):
    """ifx_magi_head_prep_kv8 in fp32 torch ops (magi_rows_util.head_prep_restatement up to the value it rounds, then the byte rule):
    two-pass statistics, w + 1 in fp32, separately rounded rotary products, x q_scale, clamp, e4m3.  `flip`: the sums in reverse order."""
    half = inp["half"]
    sin, cos = inp["rope"][:, None, :half], inp["rope"][:, None, half:]
    total = (lambda t: t.flip(-1).sum(-1, keepdim=True)) if flip else (lambda t: t.sum(-1, keepdim=True))

    def qk(t, n):
        x = t.float()
        dlt = x - total(x) * (1.0 / HD)
        y = dlt * (1.0 / torch.sqrt(total(dlt * dlt) * (1.0 / HD) + torch.tensor(U.EPS, dtype=torch.float32))) * (n[0] + 1) + n[1]
        x1, x2 = y[..., :half], y[..., half:2 * half]
        return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos, y[..., 2 * half:]], dim=-1)

    q, _, k, v = U.split_mixed(inp)
    return {"q": e4m3(qk(q, inp["qn"]) * torch.tensor(q_scale, dtype=torch.float32)), "k": e4m3(qk(k, inp["kn"])),
            "v": e4m3(v.float() / v_scale.view(1, -1, 1))}


def code_distance(a, b):      # of two e4m3 byte tensors, in representable values (+0 and -0 coincide)
    o = lambda t: torch.where(t >= 128, -(t.int() - 128), t.int())
    return (o(a) - o(b)).abs()


CAP = 0.02      # the share of elements the bf16 kernel's oracle test lets differ by one step (magi_rows_util.judge: max_mismatch_frac)


@pytest.mark.parametrize("split", [0, 35, 70])
def test_head_prep_bytes(ops, split):
    rows, hq, hk, half, row0, row1, slots = 70, 3, 2, 48, 5, 100, 180
    inp = U.head_prep_inputs(rows, hq, hk, half)
    mixed = inp["mixed"].clone()
    mixed.view(rows, -1, HD)[0, 2 * hq + hk, 0] = 1e4                          # a V value beyond 448 * v_scale saturates
    inp = dict(inp, mixed=mixed)
    v_scale, q_scale = torch.tensor([2.0, 0.3]), ops.attn_q_prescale(HD)[0]      # 0.3: the IEEE division, not a reciprocal
    want, other = _restate(inp, q_scale, v_scale, False), _restate(inp, q_scale, v_scale, True)
    for name in ("q", "k"):      # the restatement alone, summed in two orders, stays inside the cap the kernel is held to
        dd = code_distance(want[name], other[name])
        assert dd.max() <= 1 and (dd > 0).float().mean() <= CAP, (name, "restatement orders")
    dev = lambda t: t.cuda()
    kw = dict(q_heads=hq, kv_heads=hk, eps=U.EPS, layernorm_1p=True, row0=row0, split=split, row1=row1, rope=dev(inp["rope"]),
              qn=tuple(map(dev, inp["qn"])), kn=tuple(map(dev, inp["kn"])), xn=tuple(map(dev, inp["xn"])), q_scale=q_scale)
    view = ops.MagiKv8View(*(torch.full((slots, hk, HD), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)), v_scale.cuda())
    q8, qx = torch.empty(rows, hq * HD, dtype=torch.uint8, device="cuda"), torch.empty(rows, hq * HD, dtype=BF, device="cuda")
    ops.magi_head_prep_kv8(dev(mixed), kv=view, q8_out=q8, qx_out=qx, **kw)
    kb, vb = (torch.empty(slots, hk, HD, dtype=BF, device="cuda") for _ in range(2))
    qb, qxb = (torch.empty(rows, hq * HD, dtype=BF, device="cuda") for _ in range(2))
    ops.magi_head_prep(dev(mixed), layout=0, k_out=kb, v_out=vb, kv_head_stride=HD, ld_kv=hk * HD, q_out=qb, qx_out=qxb, **kw)
    assert torch.equal(qx, qxb), "qx differs from ifx_magi_head_prep's"
    dest = torch.where(torch.arange(rows) < split, row0 + torch.arange(rows), row1 + torch.arange(rows) - split)
    got = {"q": q8.cpu().view(rows, hq, HD), "k": view.k.cpu()[dest], "v": view.v.cpu()[dest]}
    for name in ("q", "k", "v"):
        dd = code_distance(got[name], want[name])
        frac = (dd > 0).float().mean().item()
        print(f"head prep kv8 split {split} {name}: max code distance {dd.max().item()}, differing {frac:.5f}")
        assert dd.max() <= (0 if name == "v" else 1) and frac <= CAP, (name, dd.max(), frac)
    assert want["v"][0, 0, 0] == 0x7E                                          # 448: the saturated value
    rest = torch.ones(slots, dtype=torch.bool)
    rest[dest] = False
    assert bool((view.k.cpu()[rest] == 0xA5).all()) and bool((view.v.cpu()[rest] == 0xA5).all()), "bytes outside dest(r) changed"



# rel-L2 of the model output with the 8-bit cache against the SAME model on the bf16 cache, per forward of the golden's walk, measured on
# the first run of this test (profiles/r35_kv8_magi.md); the test allows 1.5 x: the margin covers seed-to-seed spread of the e4m3 rounding
MODEL_REL_L2 = (2.2499e-02, 2.2703e-02, 2.3213e-02)


def test_model_option_on_vs_off(ops):
    """`HipVideoDiTModel(kv_cache_dtype="fp8_e4m3")` against the default on the forwards of tests/golden/magi_model_tiny.npz (read as
    data: first two chunks / prefix + nearly-clean / read-only window): half the cache bytes, one attn_magi launch per layer and forward,
    the output within 1.5 x the measured distance from the bf16 path; the refusals."""
    import magi_block_oracle as MB
    import magi_model_oracle as MM
    from fixture_io import golden
    from test_hip_magi_model import _config
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.types import InferenceParams
    fx = golden("magi_model_tiny.npz")
    n_layers, clip, n_calls, wseed, eseed, max_tokens = [int(v) for v in fx["geom"]]
    cfg = MM.tiny_model_config()
    sd = dict(MM.init_embedder_weights(cfg, eseed))
    for li in range(n_layers):
        sd.update({f"videodit_blocks.layers.{li}.{k}": v for k, v in MB.init_layer_weights(cfg.layer, wseed + li).items()})
    outs, nbytes, launches = {}, {}, {}
    for dtype in (None, "fp8_e4m3"):
        model = HipVideoDiTModel(_config(cfg), "cuda", kv_cache_dtype=dtype)
        model.load_state_dict(sd)
        ip = InferenceParams(1, max_tokens)
        timer = ops.KernelTimer(names=("attn_magi",))
        ops.set_kernel_timer(timer)
        try:
            outs[dtype] = []
            for ci in range(n_calls):
                range_num, dn, sp, fe, di, upd = [int(v) for v in fx[f"c{ci}_flags"]]
                args = [fx[f"c{ci}_in_{k}"].cuda() for k in ("x", "t", "y", "drop", "mask", "kv_range")]
                ip.update_kv_cache = bool(upd)
                outs[dtype].append(model(*args, inference_params=ip, range_num=range_num, denoising_range_num=dn, slice_point=sp,
                                         fwd_extra_1st_chunk=bool(fe), distill_nearly_clean_chunk=bool(di)).cpu())
        finally:
            ops.set_kernel_timer(None)
        launches[dtype] = timer.summary()["attn_magi"]["launches"]
        raw = ip.kv_cache_manager.get_raw(ip.kv_cache_request, next(iter(ip.kv_cache_manager.layers(ip.kv_cache_request))))
        nbytes[dtype] = raw.numel() * raw.element_size()
    assert 2 * nbytes["fp8_e4m3"] == nbytes[None] and launches["fp8_e4m3"] == n_layers * n_calls <= launches[None]
    for ci in range(n_calls):
        rel = rel_l2(outs["fp8_e4m3"][ci], outs[None][ci])
        print(f"magi model call {ci}: 8-bit cache vs bf16 cache rel-L2 {rel:.4e} (recorded {MODEL_REL_L2[ci]:.4e})")
        assert rel <= 1.5 * MODEL_REL_L2[ci]          # (NaN compares false)
    config = _config(cfg)
    config.engine_config.cp_strategy = "cp_ulysses"
    with pytest.raises(NotImplementedError, match="cp_strategy 'none' only"):
        HipVideoDiTModel(config, "cuda", kv_cache_dtype="fp8_e4m3")
    bad = dict(sd)
    bad["videodit_blocks.layers.0.self_attention.k_layernorm.weight"] = torch.full_like(bad["videodit_blocks.layers.0.self_attention.k_layernorm.weight"], 50.0)
    with pytest.raises(ValueError, match="e4m3 range"):
        HipVideoDiTModel(_config(cfg), "cuda", kv_cache_dtype="fp8_e4m3").load_state_dict(bad)

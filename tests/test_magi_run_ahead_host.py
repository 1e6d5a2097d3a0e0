"""No GPU: the host arithmetic of `RangePlan` bit for bit against the tensor expressions it replaces in `HipVideoDiTModel` (`unique` ->
`max_seqlen_k`, the `cu_seqlens` cumsums, the nearly-clean widening, the three plans of `forward_3cfg`, the per-row rebasing of a
batched forward), on the key ranges of the MAGI goldens and of `kv_ranges.py` for a window of 4 chunks of 6 frames; and the C-ABI of
the two row kernels (`ifx_magi_patch_rows`, `ifx_magi_unpatch`): declared, exported, bound, and refusing bad arguments."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fixture_io import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden_ranges():
    out = []
    for name, pick in (("magi_model_tiny.npz", lambda k: k.endswith("_in_kv_range")), ("magi_dispatch_tiny.npz", lambda k: k.endswith("_in_kv_range")),
                       ("magi_schedule.npz", lambda k: re.fullmatch(r"c\d+_kv", k)), ("magi_kvrange.npz", lambda k: True)):
        fx = golden(name)
        for k in sorted(fx):
            v = fx[k]
            if pick(k) and isinstance(v, torch.Tensor) and v.dtype == torch.int32 and v.dim() == 2 and v.shape[1] == 2 and v.shape[0] > 0:
                out.append((f"{name}:{k}", v))
    return out


def _schedule_ranges():
    """Every step of a clip of 6 chunks in a window of 4, chunks of 6 frames (24 tokens per frame), with and without a prefix chunk."""
    from inferix_amd.magi.schedule import ChunkSchedule
    out = []
    for offset in (0, 1):
        sch = ChunkSchedule(8, 4, 6, 6, chunk_offset=offset)
        for step in range(sch.total_forward_step()):
            out.append((f"window 4 x width 6, offset {offset}, step {step}", sch.kv_range(sch.plan(step), 6 * 24, [4, 3, 2, 2], 1, "cpu")))
    return out


def test_there_are_ranges_to_check():
    g, s = _golden_ranges(), _schedule_ranges()
    assert len(g) >= 10 and len(s) >= 30, (len(g), len(s))
    assert {n.split(":")[0] for n, _ in g} >= {"magi_model_tiny.npz", "magi_dispatch_tiny.npz", "magi_schedule.npz"}


def test_max_seqlen_k_is_unique_last_minus_first():
    from inferix_amd.magi.types import RangePlan
    for name, kv in _golden_ranges() + _schedule_ranges():
        flat = torch.unique(kv, sorted=True)
        want = int((flat[-1] - flat[0]).item())
        plan = RangePlan.make(kv.numpy(), [1] * kv.shape[0])
        assert plan.max_seqlen_k == want and isinstance(plan.max_seqlen_k, int), name
        assert plan.kv_range.dtype == np.int32 and (plan.kv_range == kv.numpy()).all(), name


def test_cu_seqlens_equal_the_cumsums():
    from inferix_amd.magi.types import cu_seqlens
    for lens in ([1, 16, 3, 7], [16] * 4, [0, 5, 0], [800] * 9, [7]):
        mask = torch.zeros(len(lens), 800)
        for i, n in enumerate(lens):
            mask[i, :n] = 1
        y_index = mask.reshape(mask.shape[0], -1).sum(-1)                                  # forward_pre_process: a float sum
        want = torch.cat([y_index.new_zeros(1), y_index]).to(torch.int64).cumsum(-1).to(torch.int32)
        got = cu_seqlens(lens)
        assert got.dtype == np.int32 and got.tolist() == want.tolist()
        assert np.stack([got[:-1], got[1:]], 1).tolist() == torch.stack([want[:-1], want[1:]], 1).tolist()
    for clip, n in ((144, 5), (12150, 8), (1, 1)):
        want = torch.tensor([0] + [clip] * n).cumsum(-1).to(torch.int32)
        assert cu_seqlens([clip] * n).tolist() == want.tolist()


class _Recorder:
    """`HipVideoDiTModel`'s dispatch code on the CPU around a `forward` that records what every single-row forward is handed."""

    def __init__(self, cfg_number):
        from inferix_amd.magi.model import HipVideoDiTModel as M
        self.M = M
        self.device, self.patch_size, self.t_patch_size = torch.device("cpu"), 2, 1
        self.runtime_config = SimpleNamespace(cfg_number=cfg_number, cfg_t_range=[0.0, 0.3], prev_chunk_scales=[1.5, 1.0], text_scales=[7.5, 0.0])
        self.seen = []

    def generate_kv_range_for_uncondition(self, x):
        return self.M.generate_kv_range_for_uncondition(self, x)

    def forward_3cfg(self, *a, **k):
        return self.M.forward_3cfg(self, *a, **k)

    def forward(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None, inference_params=None, **kw):
        if x.shape[0] > 1:                                       # the row-by-row loop of the real forward
            return self.M.forward(self, x, t, y, caption_dropout_mask, xattn_mask, kv_range, inference_params, **kw)
        self.seen.append((kv_range.clone(), xattn_mask.clone(), kw.get("range_plan"), kw["denoising_range_num"]))
        return torch.zeros_like(x, dtype=torch.float32)


def _check_seen(seen, n_expected):
    assert len(seen) == n_expected, len(seen)
    for kv, mask, plan, dn in seen:
        assert plan is not None and plan.kv_range.dtype == np.int32
        assert plan.kv_range.tolist() == kv.tolist(), (plan.kv_range.tolist(), kv.tolist())
        lens = mask.reshape(mask.shape[0], -1).sum(-1).to(torch.int64).tolist()
        assert list(plan.caption_lens) == lens and len(lens) == dn
        flat = torch.unique(kv, sorted=True)
        assert plan.max_seqlen_k == int(flat[-1] - flat[0])


def _call(dn, extra, tokens_per_frame=6, cw=2, L=16):
    """x, timestep, y, mask (conditional rows (1, 16, 3, 7, ...), null rows full) and a key-range tensor of a forward of `dn` ranges."""
    from inferix_amd.magi.kv_ranges import generate_noise2clean_kvrange
    lens = [(1, 16, 3, 7, 5)[i % 5] for i in range(dn)] + [L] * dn
    mask = torch.zeros(2 * dn, 1, L)
    for i, n in enumerate(lens):
        mask[i, :, :n] = 1
    x = torch.zeros(2, 4, dn * cw, 4, 6)
    kv = generate_noise2clean_kvrange(cw * tokens_per_frame, 2, dn, [4, 3, 2, 2], 1, ([8] if extra else []) + [2] * (dn - int(extra)), 8)
    return x, torch.rand(2, dn), torch.zeros(2 * dn, 1, L, 8), mask, kv, lens


@pytest.mark.parametrize("dn,extra", [(3, False), (4, True), (1, False)])
def test_the_three_plans_of_forward_3cfg_and_the_row_rebasing(dn, extra):
    from inferix_amd.magi.types import RangePlan
    rec = _Recorder(3)
    x, t, y, mask, kv, lens = _call(dn, extra)
    kw = dict(chunk_width=2, denoising_range_num=dn, range_num=dn + 2, slice_point=2, fwd_extra_1st_chunk=extra)
    rec.M.forward_velocities(rec, x, t, y, mask, kv, SimpleNamespace(update_kv_cache=False), nearly_clean=False,
                             cfg_bins=[0] * (dn - int(extra)), range_plan=RangePlan.make(kv.numpy(), lens), **kw)
    n_dn = dn - int(extra)
    _check_seen(rec.seen, 2 + n_dn)                              # text, previous chunks, and one row per denoising chunk
    assert list(rec.seen[0][2].caption_lens) == lens[:dn] and list(rec.seen[1][2].caption_lens) == lens[dn:]
    for b, (kvb, _, plan, _) in enumerate(rec.seen[2:]):         # rebased to the row: [0, tokens of a chunk)
        assert kvb.tolist() == [[0, 12]] and plan.caption_lens == (16,)


@pytest.mark.parametrize("dn,extra", [(3, False), (4, True)])
def test_the_nearly_clean_widening_extends_the_plan(dn, extra):
    from inferix_amd.magi.types import RangePlan
    rec = _Recorder(1)
    x, t, y, mask, kv, lens = _call(dn, extra)
    kw = dict(chunk_width=2, denoising_range_num=dn, range_num=dn + 2, slice_point=2, fwd_extra_1st_chunk=extra)
    for call in (rec.M.forward_velocities, rec.M.forward_dispatcher):
        rec.seen.clear()
        more = dict(nearly_clean=True) if call is rec.M.forward_velocities else dict(distill_nearly_clean_chunk=True)
        call(rec, x, t, y, mask, kv, SimpleNamespace(update_kv_cache=False), range_plan=RangePlan.make(kv.numpy(), lens), **more, **kw)
        _check_seen(rec.seen, 1)
        kvw, _, plan, dnw = rec.seen[0]
        s0 = int(extra)
        assert dnw == dn + 1 and kvw.shape[0] == dn + 1 and kvw[-1].tolist() == [int(kv.max()), int(kv.max()) + 12]
        assert list(plan.caption_lens) == lens[:dn] + [lens[s0]]
    rec.seen.clear()                                             # and the plain conditional forward: the first half of the captions
    rec.M.forward_velocities(rec, x, t, y, mask, kv, SimpleNamespace(update_kv_cache=False), nearly_clean=False,
                             range_plan=RangePlan.make(kv.numpy(), lens), **kw)
    _check_seen(rec.seen, 1)
    assert list(rec.seen[0][2].caption_lens) == lens[:dn]


def test_without_a_plan_no_forward_gets_one():
    rec = _Recorder(3)
    x, t, y, mask, kv, _ = _call(3, False)
    rec.M.forward_velocities(rec, x, t, y, mask, kv, SimpleNamespace(update_kv_cache=False), nearly_clean=False, cfg_bins=[0] * 3,
                             chunk_width=2, denoising_range_num=3, range_num=5, slice_point=2, fwd_extra_1st_chunk=False)
    assert len(rec.seen) == 5 and all(s[2] is None for s in rec.seen)


def test_pre_process_on_a_plan_equals_pre_process_on_the_mask_on_the_cpu():
    """The host side of the product model on the CPU (torch glue, no HIP library needed): ragged captions (1, 12, 3, 7) of 12 through
    `forward_pre_process` with a `RangePlan` and without, every tensor and range equal."""
    import magi_model_oracle as MM
    from inferix_amd.magi.dit import _cross_segments
    from inferix_amd.magi.kv_ranges import generate_noise2clean_kvrange
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.types import RangePlan
    cfg = MM.tiny_model_config()
    L = cfg.layer
    mc = SimpleNamespace(num_layers=0, hidden_size=L.hidden_size, ffn_hidden_size=L.ffn_hidden_size, num_attention_heads=L.num_attention_heads,
                         num_query_groups=L.num_query_groups, kv_channels=L.kv_channels, layernorm_epsilon=L.layernorm_epsilon,
                         apply_layernorm_1p=L.apply_layernorm_1p, patch_size=cfg.patch_size, t_patch_size=cfg.t_patch_size,
                         in_channels=cfg.in_channels, out_channels=cfg.out_channels, caption_channels=cfg.caption_channels,
                         caption_max_length=cfg.caption_max_length, cond_hidden_ratio=L.cond_hidden_ratio,
                         xattn_cond_hidden_ratio=L.xattn_cond_hidden_ratio, x_rescale_factor=cfg.x_rescale_factor, half_channel_vae=cfg.half_channel_vae)
    ec = SimpleNamespace(cp_size=1, cp_strategy="none", fp8_quant=False, distill=False)
    model = HipVideoDiTModel(SimpleNamespace(model_config=mc, engine_config=ec, runtime_config=None), "cpu")
    model.load_state_dict(MM.init_embedder_weights(cfg, 5))
    dn, cap = 4, cfg.caption_max_length
    lens = (1, cap, 3, 7)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, cfg.in_channels, dn * 2, 4, 6, generator=g)
    y = torch.randn(dn, 1, cap, cfg.caption_channels, generator=g)
    mask = torch.zeros(dn, 1, cap)
    for i, n in enumerate(lens):
        mask[i, :, :n] = 1
    kv = generate_noise2clean_kvrange(2 * 6, 1, dn, [4, 3, 2, 2], 1, [8, 4, 2, 0], 8)
    args = (x, torch.rand(1, dn, generator=g), y, torch.zeros(1, dtype=torch.bool), mask, kv)
    kw = dict(range_num=dn + 1, denoising_range_num=dn, slice_point=1, fwd_extra_1st_chunk=True)
    old = model.forward_pre_process(*args, **kw)
    new = model.forward_pre_process(*args, **kw, range_plan=RangePlan.make(kv.numpy(), lens))
    for nm, a, b in zip(("x", "condition", "condition_map", "y_xattn_flat", "rope"), old[:5], new[:5]):
        assert a.dtype == b.dtype and torch.equal(a, b), nm
    assert new[3].shape[0] == sum(lens) and new[4] is old[4] and new[2] is old[2]          # the tables are shared, not rebuilt
    for f in ("q_ranges", "kv_ranges", "cu_seqlens_q", "cu_seqlens_kv"):
        a, b = getattr(old[5].cross_attn_params, f), getattr(new[5].cross_attn_params, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    assert _cross_segments(new[5].cross_attn_params) == [(tuple(q), tuple(k)) for q, k in _cross_segments(old[5].cross_attn_params)]
    co, cn = old[5].core_attn_params, new[5].core_attn_params
    assert (co.max_seqlen_q, co.max_seqlen_k) == (cn.max_seqlen_q, cn.max_seqlen_k)
    for a, b in ((co.np_q_range, cn.np_q_range), (co.np_k_range, cn.np_k_range)):
        assert a.dtype == b.dtype and a.tolist() == b.tolist()
    with pytest.raises(ValueError):
        model.forward_pre_process(*args, **kw, range_plan=RangePlan.make(kv.numpy()[:-1], lens))


# ---- the C-ABI of the two row kernels ---------------------------------------------------------------------------------------------------
def test_the_two_exports_are_declared_exported_and_bound():
    from inferix_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "inferix_hip.h")).read()
    assert re.search(r"\bint\s+ifx_magi_patch_rows\s*\(const void\* x, int32_t is_bf16, const int64_t\* dims, const int64_t\* strides", hdr)
    assert re.search(r"\bint\s+ifx_magi_unpatch\s*\(const float\* o, int64_t ld_token", hdr)
    vp, i32, f32, i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64
    assert _hip.SIGNATURES["ifx_magi_patch_rows"] == (C.c_int, [vp, i32, vp, vp, f32, i32, i32, i32, i32, vp, i64, vp])
    assert _hip.SIGNATURES["ifx_magi_unpatch"] == (C.c_int, [vp, i64] + [i32] * 9 + [f32, vp, vp])
    lib = _hip.load()                                            # raises if the library does not export a bound name
    assert lib.ifx_magi_patch_rows is not None and lib.ifx_magi_unpatch is not None
    assert int(re.search(r"#define\s+IFX_ABI_MINOR\s+(\d+)", hdr).group(1)) == _hip.ABI_MINOR == (lib.ifx_version() >> 8) & 255


def test_the_two_exports_refuse_null_pointers_and_bad_strides():
    """Every refusal comes back before anything is launched (no GPU is needed to get it): the pointers below are never dereferenced."""
    from inferix_amd import _hip
    lib = _hip.load()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    dims, strides, ptr = i64(1, 4, 3, 4, 8), i64(384, 96, 32, 8, 1), C.c_void_p(4096)

    def rows(x=ptr, bf=0, dims=dims, strides=strides, dup=0, p=(1, 2, 2), out=ptr, ld=16):
        return lib.ifx_magi_patch_rows(x, bf, dims, strides, 1.0, dup, *p, out, ld, None)

    def refused(rc, *words):
        msg = lib.ifx_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)
    for null in ("x", "dims", "strides", "out"):
        refused(rows(**{null: None}), b"ifx_magi_patch_rows", b"null")
    refused(rows(strides=i64(768, 192, 64, 16, 2)), b"the W stride must be 1")
    refused(rows(strides=i64(384, 96, -32, 8, 1)), b"stride 2 is negative")
    refused(rows(p=(1, 0, 2)), b"bad patch 1 x 0 x 2")
    refused(rows(ld=15), b"16 elements", b"ld (15)")
    refused(rows(dup=1), b"32 elements", b"ld (16)")
    refused(rows(dims=i64(70000, 4, 3, 4, 8)), b"latent dims")
    refused(rows(x=C.c_void_p(4098)), b"4-byte")
    refused(rows(x=C.c_void_p(4097), bf=1), b"2-byte")

    def unpatch(o=ptr, ld=32, n=2, c=4, keep=4, lat=(3, 2, 4), p=(1, 2, 2), div=0.5, out=ptr):
        return lib.ifx_magi_unpatch(o, ld, n, c, keep, *lat, *p, div, out, None)
    for null in ("o", "out"):
        refused(unpatch(**{null: None}), b"ifx_magi_unpatch", b"null")
    refused(unpatch(ld=31), b"ld_token (31)", b"2 x 16")
    refused(unpatch(keep=5), b"c_out 5")
    refused(unpatch(keep=0), b"c_out 0")
    refused(unpatch(p=(1, 2, 0)), b"bad patch 1 x 2 x 0")
    refused(unpatch(div=0.0), b"divisor 0")
    refused(unpatch(lat=(3, -1, 4)), b"latent shape")
    refused(unpatch(out=C.c_void_p(4098)), b"4-byte aligned")


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    with pytest.raises(_hip.HipKernelError):
        ops.magi_patch_rows(torch.zeros(1, 4, 3, 4, 8), (1, 2, 2))           # a CPU tensor
    with pytest.raises(TypeError):
        ops.magi_patch_rows(torch.zeros(1, 4, 3, 4, 8, dtype=torch.float16), (1, 2, 2))
    with pytest.raises(ValueError):
        ops.magi_unpatch(torch.zeros(23, 1, 16), (3, 2, 4), (1, 2, 2))      # 23 tokens for a 3 x 2 x 4 latent

"""GPU: a MAGI request enqueued ahead of the device with the REAL model.  `ChunkSchedule.walk` hands `HipVideoDiTModel` a `RangePlan`
per forward (key ranges and caption lengths as the host knows them); the model then builds its packed ranges, `y_xattn_flat` and the
cross-attention segments without reading the device, keeps its tables (rope, condition map, sinusoid frequencies), and moves the latents
in and out of token rows with `ifx_magi_patch_rows` / `ifx_magi_unpatch`.  Checked here: no host synchronisation between the first
forward and the last integrate, the same bits as the path that reads the device, ragged captions, the memo tables, and the two kernels
against the torch chains they replace.

All-zero-length captions are left out: the reference never produces one (the tokenizer always emits the end-of-sequence token, and the
null caption is full length)."""
import dataclasses
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
CAP_L = 16
CHUNKS, CW, HL, WL = 4, 2, 8, 12            # 4 chunks x 2 latent frames of 8 x 12: 24 tokens per frame
LENS = (1, 16, 3, 7)                        # caption lengths of the four chunks: a single token, full, odd, odd


@functools.lru_cache(maxsize=None)
def _weights():
    import magi_block_oracle as MB
    import magi_model_oracle as MM
    cfg = dataclasses.replace(MM.tiny_model_config(), caption_max_length=CAP_L)
    sd = dict(MM.init_embedder_weights(cfg, 5))
    for li in range(cfg.num_layers):
        sd.update({f"videodit_blocks.layers.{li}.{k}": v for k, v in MB.init_layer_weights(cfg.layer, 40 + li).items()})
    return cfg, sd


def _model(cfg_number=1):
    from inferix_amd.magi.model import HipVideoDiTModel
    from test_hip_magi_model import _config
    cfg, sd = _weights()
    config = _config(cfg)
    config.engine_config.shortcut_mode = "8,16,16"
    config.engine_config.distill_nearly_clean_chunk_threshold = 0.3
    config.runtime_config = SimpleNamespace(cfg_number=cfg_number, noise2clean_kvrange=[4, 3, 2, 2], clean_chunk_kvrange=1, clean_t=0.9999,
                                            cfg_t_range=[0.0, 0.3], prev_chunk_scales=[1.5, 1.0], text_scales=[7.5, 0.0])
    model = HipVideoDiTModel(config, "cuda")
    model.load_state_dict(sd)
    return cfg, model


def _request(cfg, cfg_number, with_prefix):
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(1, cfg.in_channels, CHUNKS * CW, HL, WL, generator=g)
    y = torch.randn(2, CHUNKS, CAP_L, cfg.caption_channels, generator=g)
    masks = torch.zeros(2, CHUNKS, CAP_L)
    for c, n in enumerate(LENS):
        masks[0, c, :n] = 1
    masks[1, :, :(CAP_L if cfg_number == 3 else 2)] = 1            # the null caption: full length under guidance
    prefix = None
    if with_prefix:
        p0 = torch.randn(1, cfg.in_channels, CW + 1, HL, WL, generator=g)
        prefix = torch.cat([p0, p0], 0).cuda()
    return torch.cat([x0, x0], 0).cuda(), y.cuda(), masks.cuda(), prefix


def _walk(cfg_number, with_prefix, host_plans, on_grid=None):
    """One clip through `walk` on a fresh model and cache -> (clip, [KV cache rows per layer], nearly-clean flags)."""
    from inferix_amd.magi.schedule import ChunkSchedule
    from inferix_amd.magi.types import InferenceParams
    cfg, model = _model(cfg_number)
    x, y, masks, prefix = _request(cfg, cfg_number, with_prefix)
    tokens = CW * (HL // 2) * (WL // 2)
    ip = InferenceParams(1, CHUNKS * tokens)
    for layer in model.videodit_blocks.layers:
        # the cache is allocated uninitialised, and a row no step stores (the last chunk under guidance: its last steps are nearly clean)
        # would compare allocator garbage: allocate it here, with room for the widest forward's unstored rows, and clear it
        m = layer.self_attention.kv_cache_manager
        m.allocate_key_value_memory(ip, ip.max_sequence_length, 1, torch.bfloat16, scratch_rows=(CHUNKS + 2) * tokens)
        ip.kv_cache_manager.get_raw(ip.kv_cache_request, m.layer_name).zero_()
    nearly = []
    fv = model.forward_velocities

    def forward_velocities(**kw):
        nearly.append(bool(kw["nearly_clean"]))
        assert ("range_plan" in kw) == host_plans
        return fv(**kw)
    model.forward_velocities = forward_velocities
    sch = ChunkSchedule(8, 4, CHUNKS, CW, chunk_offset=1 if with_prefix else 0)
    handed = [i for i, _ in sch.walk(model, x, y, masks, ip, prefix_video=prefix, host_plans=host_plans)]
    if on_grid is not None:
        on_grid()                                                   # leave the sync debug mode before anything is read back
    assert handed == list(range(CHUNKS - (1 if with_prefix else 0)))
    caches = []
    for layer in model.videodit_blocks.layers:
        raw = ip.kv_cache_manager.get_raw(ip.kv_cache_request, layer.self_attention.kv_cache_manager.layer_name)
        caches.append(raw[:, :CHUNKS * tokens].clone())
    return x, caches, nearly


CASES = [(1, False), (1, True), (3, False), (3, True)]


@pytest.mark.parametrize("cfg_number,with_prefix", CASES)
def test_walk_with_the_real_model_does_not_wait_for_the_device(monkeypatch, cfg_number, with_prefix):
    """From behind the clip's one host copy (`host_grid`: time grid and caption lengths) to the last integrate, every wait for the
    device is an error: the prefix extraction pass, the clean chunk in front (`fwd_extra_1st_chunk`), the nearly-clean widened forward
    (`cfg_number == 1`) and the three guidance forwards with their batch rows (`cfg_number == 3`), all through `HipVideoDiTModel`.
    Without the plans this raises at the `masked_select` of `forward_pre_process`."""
    from inferix_amd.magi import schedule as S
    from test_hip_magi_walk import _count_syncs
    before = torch.cuda.get_sync_debug_mode()
    probe = torch.ones(3, device="cuda").sum()
    effective = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
        except RuntimeError:
            effective = True
    finally:
        torch.cuda.set_sync_debug_mode(before)
    counted = []
    if not effective:                                      # the mode does nothing on this build: count the synchronising calls instead
        _count_syncs(monkeypatch, counted)
    print("sync check by", "torch.cuda.set_sync_debug_mode('error')" if effective else "counting wrapped synchronising calls")
    grid, copies = S.host_grid, []

    def host_grid(*a):
        out = grid(*a)
        copies.append(1)
        counted.clear()
        if effective:
            torch.cuda.set_sync_debug_mode("error")        # from here on a wait for the device raises
        return out
    monkeypatch.setattr(S, "host_grid", host_grid)
    snapshot = []

    def leave():
        snapshot.extend(counted)
        torch.cuda.set_sync_debug_mode(before)
    try:
        clip, _, nearly = _walk(cfg_number, with_prefix, True, on_grid=leave)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert copies == [1] and not snapshot, snapshot
    assert True in nearly and False in nearly, nearly       # the widened forward (cfg 1) / the nearly-clean cache rule (cfg 3) is covered
    assert torch.isfinite(clip).all() and torch.equal(clip[0], clip[1])


@pytest.mark.parametrize("cfg_number,with_prefix", CASES)
def test_walk_with_plans_leaves_the_bits_of_the_walk_that_reads_the_device(cfg_number, with_prefix):
    clip, caches, nearly = _walk(cfg_number, with_prefix, True)
    clip0, caches0, nearly0 = _walk(cfg_number, with_prefix, False)
    assert nearly == nearly0
    assert torch.equal(clip, clip0), "the clip differs between the planned walk and the one that reads the ranges off the device"
    for li, (a, b) in enumerate(zip(caches, caches0)):
        assert torch.equal(a, b), f"KV cache rows of layer {li} differ"
    assert float(clip.std()) > 0.1


@pytest.mark.parametrize("cfg_number", [1, 3])
def test_ragged_captions_from_the_plan_equal_what_the_mask_gives(cfg_number):
    """One forward's pre-processing over four ranges whose captions hold (1, 16, 3, 7) of 16 tokens (the null-caption rows of a guidance
    batch: full length): `y_xattn_flat`, the packed cross-attention tensors, the segments the layers iterate and the core-attention
    ranges from the `RangePlan` against the ones read from the mask."""
    from inferix_amd.magi.dit import _cross_segments
    from inferix_amd.magi.kv_ranges import generate_default_kvrange
    from inferix_amd.magi.types import RangePlan
    cfg, model = _model(cfg_number)
    x, y, masks, _ = _request(cfg, cfg_number, False)
    dn = CHUNKS
    tokens = CW * (HL // 2) * (WL // 2)
    kv = generate_default_kvrange(tokens, 0, dn)
    t = torch.linspace(0.1, 0.9, dn).reshape(1, dn).cuda()
    rows = slice(0, 1) if cfg_number == 1 else slice(1, 2)
    lens = LENS if cfg_number == 1 else (CAP_L,) * dn
    kw = dict(range_num=dn, denoising_range_num=dn, slice_point=0, fwd_extra_1st_chunk=False)
    args = (x[0:1], t, y[rows].flatten(0, 1).unsqueeze(1), torch.zeros(1, dtype=torch.bool, device="cuda"),
            masks[rows].flatten(0, 1).unsqueeze(1), kv.cuda())
    old = model.forward_pre_process(*args, **kw)
    new = model.forward_pre_process(*args, **kw, range_plan=RangePlan.make(kv.numpy(), lens))
    for nm, a, b in zip(("x", "condition", "condition_map", "y_xattn_flat", "rope"), old[:5], new[:5]):
        assert a.dtype == b.dtype and torch.equal(a, b), nm
    assert new[3].shape[0] == sum(lens)
    mo, mn = old[5], new[5]
    for f in ("q_ranges", "kv_ranges", "cu_seqlens_q", "cu_seqlens_kv"):
        a, b = getattr(mo.cross_attn_params, f), getattr(mn.cross_attn_params, f)
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), f
    assert mo.cross_attn_params.host_q_ranges is None and mn.cross_attn_params.host_kv_ranges is not None
    assert [(tuple(q), tuple(k)) for q, k in _cross_segments(mo.cross_attn_params)] == \
        [(tuple(q), tuple(k)) for q, k in _cross_segments(mn.cross_attn_params)]
    co, cn = mo.core_attn_params, mn.core_attn_params
    assert co.max_seqlen_k == cn.max_seqlen_k and co.max_seqlen_q == cn.max_seqlen_q
    assert co.np_q_range.dtype == cn.np_q_range.dtype and (co.np_q_range == cn.np_q_range).all()
    assert co.np_k_range.dtype == cn.np_k_range.dtype and (co.np_k_range == cn.np_k_range).all()
    with pytest.raises(ValueError):                             # a plan of another forward
        model.forward_pre_process(*args, **kw, range_plan=RangePlan.make(kv.numpy(), lens[:-1]))


def test_tables_are_made_once_and_stay_bounded():
    from inferix_amd.magi import model as M
    from inferix_amd.magi.kv_ranges import generate_default_kvrange
    cfg, model = _model(1)
    x, y, masks, _ = _request(cfg, 1, False)
    tokens = CW * (HL // 2) * (WL // 2)

    def pre(dn, slice_point=0):
        kv = generate_default_kvrange(tokens, slice_point, dn).cuda()
        t = torch.full((1, dn), 0.5, device="cuda")
        return model.forward_pre_process(x[0:1, :, :dn * CW], t, y[0, :dn].unsqueeze(1), torch.zeros(1, dtype=torch.bool, device="cuda"),
                                         masks[0, :dn].unsqueeze(1), kv, range_num=slice_point + dn, denoising_range_num=dn,
                                         slice_point=slice_point, fwd_extra_1st_chunk=False)
    a, b = pre(2), pre(2)
    assert a[4] is b[4] and a[2] is b[2], "two forwards of one geometry must share the rope table and the condition map"
    assert a[4] is model._rope(2 * CW, HL // 2, WL // 2, 2 * tokens)
    c = pre(2, slice_point=1)                                   # the same rows of a longer clip: t_total changes
    assert c[4] is not a[4] and c[4].shape == a[4].shape and not torch.equal(c[4], a[4])
    assert torch.equal(a[4], model._build_rope(2 * CW, HL // 2, WL // 2, 2 * tokens))
    freqs = model._t_freqs
    pre(3)
    assert model._t_freqs is freqs and freqs is not None
    for t_total in range(1, 3 * M.MEMO_BOUND):
        model._rope(t_total, 2, 2, 4)
    assert len(model._rope_memo) == M.MEMO_BOUND
    assert model._rope(3 * M.MEMO_BOUND - 1, 2, 2, 4) is model._rope(3 * M.MEMO_BOUND - 1, 2, 2, 4)


# ---- the two row kernels against the torch chains of forward_pre_process / forward_post_process ------------------------------------------
def _patch_chain(x, factor, dup, pt, pp):
    x = x * factor
    if dup:
        x = torch.cat([x, x], dim=1)
    x = x.float()
    N, C, Tf, Hf, Wf = x.shape
    T, H, Wd = Tf // pt, Hf // pp, Wf // pp
    return x[:, :, :T * pt, :H * pp, :Wd * pp].reshape(N, C, T, pt, H, pp, Wd, pp).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N, T * H * Wd, -1)


def _unpatch_chain(o, T, H, Wd, pt, p, C, keep, factor):
    S, N, _ = o.shape
    o = o.reshape(T, H, Wd, N, pt, p, p, C).permute(3, 7, 0, 4, 1, 5, 2, 6).reshape(N, C, T * pt, H * p, Wd * p).contiguous()
    if keep is not None:
        o = o[:, :keep]
    return o / factor


SHAPES = [(4, 8), (6, 10), (5, 7)]       # 16-byte path; kept width 10: 4-byte path; trailing row and column dropped (kept 4 x 6: 4-byte)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("n,dup", [(1, False), (2, True), (2, False), (1, True)])
def test_patch_rows_equal_the_torch_chain(n, dup, hw, dtype):
    from inferix_amd import hip_ops as ops
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1] + n)
    x = torch.randn(n, 4, 3, *hw, generator=g).to(dtype).cuda()
    factor = 0.7                                                 # not a power of two: the product rounds
    want = _patch_chain(x, factor, dup, 1, 2)
    got = ops.magi_patch_rows(x, (1, 2, 2), factor, dup)
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    # a canary row behind the rows: nothing is written past them
    buf = torch.full((want.numel() + want.shape[-1],), -7.0, device="cuda")
    ops.magi_patch_rows(x, (1, 2, 2), factor, dup, out=buf[:want.numel()].view(want.shape))
    assert torch.equal(buf[:want.numel()].view(want.shape), want) and bool((buf[want.numel():] == -7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_patch_rows_read_a_frame_window_in_place_and_refuse_a_strided_w_axis(dtype):
    """Pinned: a view whose W axis is contiguous (a frame window, a batch row, a channel slice of a larger tensor) is read in place;
    a view whose W stride is not 1 is refused (IFX_EINVAL in the library, ValueError in the wrapper)."""
    import ctypes as C
    from inferix_amd import _hip
    from inferix_amd import hip_ops as ops
    big = torch.randn(3, 6, 5, 4, 8, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    view = big[1:3, 1:5, 1:4]
    assert not view.is_contiguous()
    assert torch.equal(ops.magi_patch_rows(view, (1, 2, 2), 0.7, True), _patch_chain(view, 0.7, True, 1, 2))
    odd = big[1:2, :, 1:3, 1:4, 1:8]                             # rows start off the 16-byte grid: the 4-byte path, same rows
    assert torch.equal(ops.magi_patch_rows(odd, (1, 2, 2), 0.7, False), _patch_chain(odd, 0.7, False, 1, 2))
    strided = big[..., ::2]
    with pytest.raises(ValueError):
        ops.magi_patch_rows(strided, (1, 2, 2))
    out = torch.zeros(3 * 5 * 2 * 2, 24, device="cuda")
    dims, strides = (C.c_int64 * 5)(*strided.shape), (C.c_int64 * 5)(*strided.stride())
    rc = _hip.load().ifx_magi_patch_rows(strided.data_ptr(), int(dtype == torch.bfloat16), dims, strides, 1.0, 0, 1, 2, 2, out.data_ptr(), 24, None)
    assert rc == -1 and b"W stride" in _hip.load().ifx_last_error()
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("hw", [(2, 4), (3, 5), (2, 3)])     # result widths 8 (16-byte stores), 10 and 6 (4-byte stores)
@pytest.mark.parametrize("n,channels,keep", [(1, 4, None), (2, 4, None), (2, 8, 4), (1, 8, 4)])
def test_unpatch_equals_the_torch_chain(n, channels, keep, hw):
    from inferix_amd import hip_ops as ops
    T, (H, Wd), pt, p = 3, hw, 1, 2
    g = torch.Generator().manual_seed(H * 10 + Wd + n)
    o = torch.randn(T * H * Wd, n, pt * p * p * channels, generator=g).cuda()
    factor = 0.7
    want = _unpatch_chain(o, T, H, Wd, pt, p, channels, keep, factor)
    got = ops.magi_unpatch(o, (T, H, Wd), (pt, p, p), factor, keep)
    assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.magi_unpatch(o, (T, H, Wd), (pt, p, p), factor, channels + 1)

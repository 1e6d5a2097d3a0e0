"""GPU: the MAGI layer and model with the gated MLP (`gated_linear_unit`: the 24B configs) on the HIP path, against the fixtures the
reference's own gated `TransformerLayer` produced on the CPU (tools/gen_golden_magi_gated.py) and against the CPU restatements
(oracle/magi_block_oracle.py, oracle/magi_model_oracle.py, pinned to the reference by tests/test_magi_gated_oracle.py and the
magi_model_tiny fixture).  Procedures and bars are those of the ungated tests in tests/test_hip_magi_block.py and
tests/test_hip_magi_model.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import magi_block_oracle as MB
import magi_model_oracle as MM
from magi_gated_util import gated_geometry, gated_golden
from util import assert_bf16_parity, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _configs(cfg: MB.MagiLayerConfig, n_layers: int, fp8: bool = False):
    mc = SimpleNamespace(num_layers=max(n_layers, 3), hidden_size=cfg.hidden_size, ffn_hidden_size=cfg.ffn_hidden_size,
                         num_attention_heads=cfg.num_attention_heads, num_query_groups=cfg.num_query_groups,
                         kv_channels=cfg.kv_channels, layernorm_epsilon=cfg.layernorm_epsilon,
                         apply_layernorm_1p=cfg.apply_layernorm_1p, gated_linear_unit=cfg.gated_linear_unit, params_dtype=BF)
    ec = SimpleNamespace(cp_size=1, cp_strategy="none", fp8_quant=fp8, kv_offload=False, ulysses_overlap_degree=1)
    return mc, ec


def _meta(m: MB.LayerMeta):
    from inferix_amd.magi.types import ModelMetaArgs, PackedCoreAttnParams, PackedCrossAttnParams
    qr, kr = torch.tensor(m.q_ranges, dtype=torch.int32), torch.tensor(m.k_ranges, dtype=torch.int32)
    core = PackedCoreAttnParams(q_range=qr, k_range=kr, np_q_range=qr.numpy(), np_k_range=kr.numpy(),
                                max_seqlen_q=m.clip_token_nums, max_seqlen_k=int(kr[:, 1].max()))
    cross = PackedCrossAttnParams(cu_seqlens_q=torch.tensor(m.cu_seqlens_q, dtype=torch.int32),
                                  cu_seqlens_kv=torch.tensor(m.cu_seqlens_kv, dtype=torch.int32),
                                  max_seqlen_q=m.clip_token_nums, max_seqlen_kv=int(np.diff(m.cu_seqlens_kv).max()))
    return ModelMetaArgs(H=1, W=1, cp_pad_size=0, cp_split_sizes=None, slice_point=m.slice_point,
                         denoising_range_num=len(m.q_ranges), range_num=len(m.q_ranges) + m.slice_point,
                         extract_prefix_video_feature=False, fwd_extra_1st_chunk=m.use_cache and m.slice_point == 0,
                         distill_nearly_clean_chunk=m.distill_nearly_clean_chunk, clip_token_nums=m.clip_token_nums,
                         enable_cuda_graph=False, core_attn_params=core, cross_attn_params=cross)


@pytest.mark.parametrize("name", ["magi_block_gated_tiny", "magi_block_24b"])
def test_gated_layer_stack_vs_reference_golden(name):
    """test_layer_stack_vs_reference_golden with the gated MLP: two stacked tiny layers over the four forwards of the cache rule, and
    ONE layer at the 24B dimensions (hidden 6144: the 12-chunk LayerNorm and gate-norm kernels, 48 q-heads on 8 groups, fc1 of
    32768 rows, silu_and_mul at f = 16384).  Layer 0 sees identical inputs: within 1.25 x the reference's own distance from the
    float64 layer (+ 5e-4) of that evaluation, elementwise within 8 ULP; chained layers < 1e-2; cache K at 1 ULP, V at 2."""
    from inferix_amd.magi.dit import HipMagiTransformerLayer
    from inferix_amd.magi.types import InferenceParams
    fx = gated_golden(name)
    cfg, n_layers, clip, n_calls, wseed, max_tokens = gated_geometry(fx)
    mc, ec = _configs(cfg, n_layers)
    Ws = [MB.init_layer_weights(cfg, wseed + li) for li in range(n_layers)]
    layers = []
    for li in range(n_layers):
        layer = HipMagiTransformerLayer(mc, ec, li, "cuda")
        layer.load_state_dict(Ws[li])
        layers.append(layer)
    ip = InferenceParams(1, max_tokens)
    orc_caches = [MB.MagiLayerCache(max_tokens, cfg.num_query_groups, cfg.kv_channels) for _ in range(n_layers)]
    for ci in range(n_calls):
        inp, m = MB.fixture_call(fx, ci)
        meta = _meta(m)
        ip.update_kv_cache = m.update_kv_cache
        x = inp["x"].cuda()
        x_ref = inp["x"]
        for li, layer in enumerate(layers):
            # yardstick: the float64 layer on the REFERENCE's input of this layer, with the reference's cache prefix
            exact = MB.exact_layer_forward(Ws[li], cfg, x_ref, inp["condition"], inp["condition_map"], inp["y"], inp["rope"], m,
                                           orc_caches[li])
            ref = fx[f"c{ci}_out_l{li}"]
            x = layer(x, inp["condition"].cuda(), inp["condition_map"].cuda(), inp["y"].cuda(), inp["rope"].cuda(), ip, meta)
            if li == 0:                       # identical inputs on both sides: the per-layer bar
                floor = rel_l2(ref, exact)
                d_hip_exact, d_hip_ref = rel_l2(x.cpu(), exact), rel_l2(x.cpu(), ref)
                print(f"{name} call {ci} layer 0: ref-vs-exact {floor:.3e}  hip-vs-exact {d_hip_exact:.3e}  hip-vs-ref {d_hip_ref:.3e}")
                assert d_hip_exact <= 1.25 * floor + 5e-4, (ci, d_hip_exact, floor)
                assert_bf16_parity(x, ref, max_ulp=8, max_mismatch_frac=0.6, rel=2.0 * floor + 5e-4, floor=1.0,
                                   what=f"{name} call {ci} layer 0")
            else:                             # chained layers: inputs already differ by the floor
                assert rel_l2(x.cpu(), ref) < 1e-2, (ci, li)
            # advance the oracle's cache with the reference's own stream so the yardstick prefix stays the reference's
            MB.layer_forward(Ws[li], cfg, x_ref, inp["condition"], inp["condition_map"], inp["y"], inp["rope"], m, orc_caches[li])
            x_ref = ref
    written = int(fx["cache_written"])
    for li in range(n_layers):
        raw = ip.kv_cache_manager.get_raw(ip.kv_cache_request, f"layer_{li}")
        if li == 0:
            assert_bf16_parity(raw[0, :written, 0], fx[f"cache_l{li}"][0, :written, 0], max_ulp=1, floor=1.0, max_mismatch_frac=0.05,
                               what="cache K (LayerNorm + rotary)")
            assert_bf16_parity(raw[1, :written, 0], fx[f"cache_l{li}"][1, :written, 0], max_ulp=2, floor=0.05, what="cache V")
        else:
            assert rel_l2(raw[:, :written].cpu(), fx[f"cache_l{li}"][:, :written]) < 1e-2


def test_gated_fp8_quant_layer_stack_vs_reference_golden():
    """test_fp8_quant_layer_stack_vs_reference_golden with the gated MLP: three layers, the middle one on the static-scale FP8 linears
    — there fc1's bf16 output goes through ifx_silu_and_mul, which writes fc2's quantised input.  Every layer gets the REFERENCE's input
    (teacher forcing).  bf16 layers < 6e-3; the FP8 layer closer to the reference than the reference layer's own response to a
    1-ULP nudge of 5 % of its input elements (computed here from the oracle, asserted > 8e-3), 2e-2 on the later calls; cache < 1.5e-2."""
    from inferix_amd.magi.dit import HipMagiTransformerLayer
    from inferix_amd.magi.types import InferenceParams
    fx = gated_golden("magi_block_gated_fp8_tiny")
    assert int(fx["fp8_quant"]) == 1
    cfg, n_layers, clip, n_calls, wseed, max_tokens = gated_geometry(fx)
    mc, ec = _configs(cfg, n_layers, fp8=True)
    layers, Ws = [], []
    for li in range(n_layers):
        layer = HipMagiTransformerLayer(mc, ec, li, "cuda")
        Ws.append(MB.init_layer_weights(cfg, wseed + li, fp8=MB.layer_is_fp8(li, mc.num_layers)))
        layer.load_state_dict(Ws[li])
        assert layer.gated and bool(layer.fp8) == (li == 1) and bool(layer.self_attention.fp8) == (li == 1)
        layers.append(layer)
    with pytest.raises(ValueError, match="fc1"):           # an ungated checkpoint (fc1 of f rows) in a layer the config says is gated
        import dataclasses
        HipMagiTransformerLayer(mc, ec, 0, "cuda").load_state_dict(MB.init_layer_weights(dataclasses.replace(cfg, gated_linear_unit=False), wseed))
    ip = InferenceParams(1, max_tokens)
    g = torch.Generator().manual_seed(0)
    for ci in range(n_calls):
        inp, m = MB.fixture_call(fx, ci)
        meta = _meta(m)
        ip.update_kv_cache = m.update_kv_cache
        x_in = inp["x"]
        for li, layer in enumerate(layers):
            ref = fx[f"c{ci}_out_l{li}"]
            got = layer(x_in.cuda(), inp["condition"].cuda(), inp["condition_map"].cuda(), inp["y"].cuda(), inp["rope"].cuda(), ip, meta)
            r = rel_l2(got.cpu(), ref)
            bar = 6e-3
            if li == 1 and ci == 0:                          # the reference layer's own response to a 1-ULP nudge of 5 % of its input
                xi = x_in.view(torch.int16).clone()
                mask = torch.rand(x_in.shape, generator=g) < 0.05
                xi[mask] += (torch.randint(0, 2, x_in.shape, generator=g) * 2 - 1).to(torch.int16)[mask]
                cache = MB.MagiLayerCache(max_tokens, cfg.num_query_groups, cfg.kv_channels)
                nudged = MB.layer_forward(Ws[1], cfg, xi.view(BF), inp["condition"], inp["condition_map"], inp["y"], inp["rope"], m, cache)
                bar = rel_l2(nudged, ref)
                assert bar > 8e-3, bar                       # the yardstick really is of that size
            elif li == 1:
                bar = 2e-2
            print(f"gated fp8 stack call {ci} layer {li} ({'fp8' if li == 1 else 'bf16'}): hip-vs-ref {r:.3e}  (bar {bar:.3e})")
            assert r < bar, (ci, li, r, bar)
            x_in = ref
    written = int(fx["cache_written"])
    raw = ip.kv_cache_manager.get_raw(ip.kv_cache_request, "layer_1")           # K / V of the FP8 layer: fp8 GEMM outputs
    assert rel_l2(raw[:, :written].cpu(), fx["cache_l1"][:, :written]) < 1.5e-2


# ---------------------------------------------------------------------------------------------------------------------------------
def _model_config(cfg: MM.MagiModelConfig):
    """The reference's ModelConfig fields for `cfg`.  `in_channels` is the reference's: the input width of the patch embedding, i.e.
    with half_channel_vae the 16 latent channels concatenated with themselves (dit_model.py:66-72, :270-272; 32 in the 24B configs),
    which oracle/magi_model_oracle.py writes as `in_channels` (the latent channels) x 2."""
    L = cfg.layer
    mc = SimpleNamespace(num_layers=cfg.num_layers, hidden_size=L.hidden_size, ffn_hidden_size=L.ffn_hidden_size,
                         num_attention_heads=L.num_attention_heads, num_query_groups=L.num_query_groups, kv_channels=L.kv_channels,
                         layernorm_epsilon=L.layernorm_epsilon, apply_layernorm_1p=L.apply_layernorm_1p,
                         gated_linear_unit=L.gated_linear_unit, params_dtype=BF, patch_size=cfg.patch_size, t_patch_size=cfg.t_patch_size,
                         in_channels=cfg.in_channels * (2 if cfg.half_channel_vae else 1), out_channels=cfg.out_channels,
                         caption_channels=cfg.caption_channels, caption_max_length=cfg.caption_max_length,
                         cond_hidden_ratio=L.cond_hidden_ratio, xattn_cond_hidden_ratio=L.xattn_cond_hidden_ratio,
                         cond_gating_ratio=L.cond_gating_ratio, x_rescale_factor=cfg.x_rescale_factor, half_channel_vae=cfg.half_channel_vae)
    ec = SimpleNamespace(cp_size=1, cp_strategy="none", fp8_quant=False, kv_offload=False, ulysses_overlap_degree=1, distill=False)
    return SimpleNamespace(model_config=mc, engine_config=ec, runtime_config=None)


def test_model_with_24b_shaped_tiny_config_vs_oracle_model():
    """`HipVideoDiTModel` needs nothing new for the 24B configs; this proves it on a tiny config with their shape: gated layers,
    half_channel_vae (16 latent channels doubled into a 32-channel patch embedding), 32 output channels of which 16 are kept,
    x_rescale_factor 0.1.  Two forwards that walk the cache rule (store two chunks, then prefix + store) against the CPU restatement
    of the model (pre_process, MB.layer_forward per layer, post_process); the yardstick is the same model with float64 layers, as
    `_exact_model` of tests/test_hip_magi_model.py: the restatement sits `floor` from it, the HIP result within 1.25 x floor + 5e-4 of both.
    The oracle's config counts the LATENT channels as `in_channels` (16 here; its patch embedding has 2 x 16 = 32 input channels, the
    reference's `in_channels = 32`), see `_model_config`."""
    import dataclasses
    from inferix_amd.magi.model import HipVideoDiTModel
    from inferix_amd.magi.types import InferenceParams
    L = dataclasses.replace(MB.tiny_config(), gated_linear_unit=True)
    cfg = MM.MagiModelConfig(layer=L, num_layers=3, in_channels=16, out_channels=32, half_channel_vae=True, x_rescale_factor=0.1,
                             caption_channels=64, caption_max_length=12)
    config = _model_config(cfg)
    assert config.model_config.in_channels == 32 and config.model_config.out_channels == 32
    EW = MM.init_embedder_weights(cfg, 31)
    Ws = [MB.init_layer_weights(L, 1100 + li) for li in range(cfg.num_layers)]
    sd = dict(EW)
    for li, W in enumerate(Ws):
        sd.update({f"videodit_blocks.layers.{li}.{k}": v for k, v in W.items()})
    model = HipVideoDiTModel(config, "cuda")
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(32)
    Hl, Wl, Lc, Cc = 8, 12, cfg.caption_max_length, cfg.caption_channels
    clip = (Hl // cfg.patch_size) * (Wl // cfg.patch_size)
    max_tokens = 4 * clip
    calls = []
    for kv, caps, drop, kw in (([(0, clip), (0, 2 * clip)], (7, 5), False,
                                dict(range_num=2, denoising_range_num=2, slice_point=0, fwd_extra_1st_chunk=True)),
                               ([(0, 2 * clip), (0, 3 * clip)], (12, 3), True,
                                dict(range_num=3, denoising_range_num=2, slice_point=1, fwd_extra_1st_chunk=False,
                                     distill_nearly_clean_chunk=True))):
        mask = torch.zeros(2, 1, 1, Lc)
        for r, c in enumerate(caps):
            mask[r, ..., :c] = 1
        calls.append(dict(x=torch.randn(1, 16, 2, Hl, Wl, generator=g), t=torch.rand(1, 2, generator=g),
                          y=torch.randn(2, 1, Lc, Cc, generator=g), mask=mask, kv_range=torch.tensor(kv, dtype=torch.int32),
                          drop=torch.tensor([drop]), kw=kw))
    ip = InferenceParams(1, max_tokens)
    ip.update_kv_cache = True
    bf_caches = [MB.MagiLayerCache(max_tokens, L.num_query_groups, L.kv_channels) for _ in Ws]
    for ci, c in enumerate(calls):
        kw = c["kw"]
        xs, cond, cmap, yf, rope, meta = MM.pre_process(EW, cfg, c["x"], c["t"], c["y"], c["mask"], c["kv_range"], c["drop"],
                                                        range_num=kw["range_num"], denoising_range_num=kw["denoising_range_num"],
                                                        slice_point=kw["slice_point"])
        lm = MB.LayerMeta(q_ranges=[tuple(r) for r in meta["q_range"].tolist()], k_ranges=[tuple(r) for r in c["kv_range"].tolist()],
                          cu_seqlens_q=meta["cu_seqlens_q"].tolist(), cu_seqlens_kv=meta["cu_seqlens_kv"].tolist(),
                          clip_token_nums=meta["clip_token_nums"], slice_point=kw["slice_point"], update_kv_cache=True,
                          use_cache=bool(kw["fwd_extra_1st_chunk"]) or kw["slice_point"] > 0,
                          distill_nearly_clean_chunk=bool(kw.get("distill_nearly_clean_chunk", False)))
        # the float64 layers READ the cache the bf16 restatement keeps: exact layer first (the prefix as stored before this forward)
        h, h_bf = xs, xs
        for W, cache in zip(Ws, bf_caches):
            h = MB.exact_layer_forward(W, L, h, cond, cmap, yf, rope, lm, cache)
            h_bf = MB.layer_forward(W, L, h_bf, cond, cmap, yf, rope, lm, cache)
        exact = MM.post_process(EW, cfg, h.float(), meta["H"], meta["W"])
        ref = MM.post_process(EW, cfg, h_bf.float(), meta["H"], meta["W"])
        out = model(c["x"].cuda(), c["t"].cuda(), c["y"].cuda(), c["drop"].cuda(), c["mask"].cuda(), c["kv_range"].cuda(),
                    inference_params=ip, **kw).cpu()
        assert out.shape == ref.shape == (1, 16, 2, Hl, Wl) and out.dtype == torch.float32
        floor, mine, r = rel_l2(ref, exact), rel_l2(out, exact), rel_l2(out, ref)
        print(f"24B-shaped tiny model call {ci}: floor (restatement vs float64 layers) {floor:.3e}; HIP vs float64 {mine:.3e}; HIP vs restatement {r:.3e}")
        assert mine <= 1.25 * floor + 5e-4 and r <= 1.25 * floor + 5e-4, (ci, floor, mine, r)
    # the synthetic weights of the same settings load and run (benchmarks and smoke runs have no checkpoint)
    synth = HipVideoDiTModel(config, "cuda")
    synth.load_synthetic(seed=3)
    c = calls[0]
    o = synth(c["x"].cuda(), c["t"].cuda(), c["y"].cuda(), c["drop"].cuda(), c["mask"].cuda(), c["kv_range"].cuda(),
              inference_params=InferenceParams(1, max_tokens), **c["kw"])
    assert o.shape == (1, 16, 2, Hl, Wl) and bool(torch.isfinite(o).all())

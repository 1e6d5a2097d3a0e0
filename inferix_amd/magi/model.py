"""MAGI-1 `VideoDiTModel` on MI355X: one denoise forward of the whole model (BASELINE config 5 as a MODEL step, not a layer stack).

Mirrors `inferix/models/magi/dit/dit_model.py` of the reference:
  forward_pre_process / get_embedding_and_meta :111-330   patch embedding, rope table, timestep / caption embedders, condition and
                                                          condition map, packed cross- / core-attention ranges, cp_pre_process
  forward                                      :353-398   the layer stack (HipMagiTransformerBlock: every heavy op a HIP kernel)
  TransformerBlock.forward tail                dit_module.py:1386-1388   final LayerNorm on the fp32 hidden states
  forward_post_process / unpatchify            :97-107,332-351   FinalLinear, cp_post_process, (T H W) N (pT pH pW C) -> N C T H W

What runs where.  The 34 layers are >99.9 % of a forward's arithmetic and go through inferix_amd.magi.dit (HIP GEMMs, attention,
norms).  The embedders, the rope table, the final LayerNorm and the final linear are fp32 modules upstream (`_high_precision_promoter`,
:620-637; evaluated under `torch.autocast("cuda", dtype=torch.float32)`): here they are a handful of fp32 torch calls on the device —
glue by the contract's definition (a 64-wide patchify GEMM, two-layer MLPs on one row per denoising range, an 800-row caption
projection, a 3072 -> 64 head), with the same rounding points as the reference: the sinusoid is rounded to bf16 before the fp32
timestep MLP (`t_freq.to(params_dtype)`), x / condition / y_xattn_flat are rounded to bf16 behind the embedders.

Parity: tests/test_hip_magi_model.py against tests/golden/magi_model_tiny.npz (the reference's own VideoDiTModel.forward run by
oracle/gen_golden_magi_model.py; the layers follow the reference's CPU path as the layer goldens do).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import numpy as np

from .. import hip_ops as ops
from . import context_parallel as cpl
from .dit import HipMagiTransformerBlock
from .types import InferenceParams, ModelMetaArgs, PackedCoreAttnParams, PackedCrossAttnParams, RangePlan, cu_seqlens

BF16 = torch.bfloat16
MEMO_BOUND = 16          # entries per memo table of a model (rope tables, condition maps, packed ranges); the oldest entry leaves first


def _memoised(store: dict, key, make):
    """`store[key]`, made on first use; `store` never holds more than MEMO_BOUND entries.  What comes out is shared between forwards and
    must not be written."""
    hit = store.get(key)
    if hit is None:
        if len(store) >= MEMO_BOUND:
            store.pop(next(iter(store)))
        hit = store[key] = make()
    return hit


def _upload(a: np.ndarray, device) -> torch.Tensor:
    """Host array -> device through pinned memory, without waiting for the device."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else t


def _with_plan(plan: Optional[RangePlan]) -> dict:
    return {} if plan is None else {"range_plan": plan}


def _row_tokens(model, x: torch.Tensor) -> int:
    """Tokens of one batch row of `x` `[B, C, T, H, W]`: the `n` of `generate_kv_range_for_uncondition`."""
    return (x.shape[2] // model.t_patch_size) * (x.shape[3] // model.patch_size) * (x.shape[4] // model.patch_size)


def _cfg(c, name, default):
    return getattr(c, name, default)


class HipVideoDiTModel:
    """`VideoDiTModel(config)` with `.forward(x, t, y, caption_dropout_mask, xattn_mask, kv_range, inference_params, **kwargs)`.
    `config` carries `model_config` / `engine_config` (/ `runtime_config`) as the reference's MagiConfig does."""

    def __init__(self, config, device="cuda"):
        self.model_config, self.engine_config = config.model_config, config.engine_config
        self.runtime_config = getattr(config, "runtime_config", None)
        mc = self.model_config
        self.device = torch.device(device)
        self.patch_size, self.t_patch_size = _cfg(mc, "patch_size", 2), _cfg(mc, "t_patch_size", 1)
        self.in_channels, self.out_channels = _cfg(mc, "in_channels", 16), _cfg(mc, "out_channels", 16)
        self.caption_max_length = _cfg(mc, "caption_max_length", 800)
        self.x_rescale_factor, self.half_channel_vae = float(_cfg(mc, "x_rescale_factor", 1.0)), bool(_cfg(mc, "half_channel_vae", False))
        self.frequency_embedding_size = 256
        self.videodit_blocks = HipMagiTransformerBlock(mc, self.engine_config, device)
        self.w: Dict[str, torch.Tensor] = {}
        self._rope_memo: dict = {}           # (t_total, H, W, rows, device) -> rope rows
        self._map_memo: dict = {}            # (N, dn, tokens per range) -> condition_map
        self._range_memo: dict = {}          # (dn N, clip) / caption length tuple -> packed ranges on the device + their host copies
        self._t_freqs: Optional[torch.Tensor] = None

    # ---- weights --------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, W: Dict[str, torch.Tensor]) -> None:
        """State dict with the reference's names: `x_embedder.weight`, `t_embedder.mlp.{0,2}.*`, `y_embedder.*`, `rope.bands`,
        `videodit_blocks.layers.{i}.*`, `videodit_blocks.final_layernorm.*`, `final_linear.linear.weight`."""
        dev = self.device
        for k in ("x_embedder.weight", "t_embedder.mlp.0.weight", "t_embedder.mlp.0.bias", "t_embedder.mlp.2.weight", "t_embedder.mlp.2.bias",
                  "y_embedder.null_caption_embedding", "y_embedder.y_proj_xattn.0.weight", "y_embedder.y_proj_xattn.0.bias",
                  "y_embedder.y_proj_adaln.0.weight", "y_embedder.y_proj_adaln.0.bias", "rope.bands",
                  "videodit_blocks.final_layernorm.weight", "videodit_blocks.final_layernorm.bias", "final_linear.linear.weight"):
            if k not in W:
                raise KeyError(f"HipVideoDiTModel.load_state_dict: missing {k}")
            self.w[k] = W[k].to(dev, torch.float32).contiguous()          # fp32 modules (_high_precision_promoter)
        self.videodit_blocks.load_state_dict(W, "videodit_blocks.layers.")
        self._rope_memo.clear()              # the rope table is a function of rope.bands

    def load_synthetic(self, seed: int = 0, fp8: Optional[bool] = None) -> None:
        """Random weights of the whole model with the reference's shapes and dtypes, generated on the device layer by layer (no
        checkpoint exists offline): benchmarks and smoke runs.  `fp8` (default `engine_config.fp8_quant`): layers 1 .. n - 2 carry the
        static-scale e4m3 linears of an fp8_quant checkpoint (dit_module.py:434-490)."""
        from .dit import synthetic_layer_state_dict
        mc, dev = self.model_config, self.device
        fp8 = bool(_cfg(self.engine_config, "fp8_quant", False)) if fp8 is None else fp8
        g = torch.Generator(device=dev).manual_seed(seed)
        h, heads = mc.hidden_size, mc.num_attention_heads
        cond, xat = int(h * _cfg(mc, "cond_hidden_ratio", 0.25)), int(h * _cfg(mc, "xattn_cond_hidden_ratio", 1.0))
        cin = self.in_channels          # the patch embedding's input width (dit_model.py:66-72); half_channel_vae: 2 x 16 latent channels
        cap = _cfg(mc, "caption_channels", 4096)
        rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev)
        mat = lambda *shape: rnd(*shape) * math.prod(shape[1:]) ** -0.5
        n = h // heads // 8
        bands = 1.0 / (10000.0 ** (torch.arange(0, n, dtype=torch.int64, device=dev).to(torch.float32) / n))
        self.w = {"x_embedder.weight": mat(h, cin, self.t_patch_size, self.patch_size, self.patch_size),
                  "t_embedder.mlp.0.weight": mat(cond, self.frequency_embedding_size), "t_embedder.mlp.0.bias": 0.1 * rnd(cond),
                  "t_embedder.mlp.2.weight": mat(cond, cond), "t_embedder.mlp.2.bias": 0.1 * rnd(cond),
                  "y_embedder.null_caption_embedding": rnd(self.caption_max_length, cap),
                  "y_embedder.y_proj_xattn.0.weight": mat(xat, cap), "y_embedder.y_proj_xattn.0.bias": 0.1 * rnd(xat),
                  "y_embedder.y_proj_adaln.0.weight": mat(cond, cap), "y_embedder.y_proj_adaln.0.bias": 0.1 * rnd(cond),
                  "rope.bands": bands, "videodit_blocks.final_layernorm.weight": 0.1 * rnd(h),
                  "videodit_blocks.final_layernorm.bias": 0.1 * rnd(h),
                  "final_linear.linear.weight": mat(self.patch_size * self.patch_size * self.t_patch_size * self.out_channels, h)}
        self._rope_memo.clear()
        layers = self.videodit_blocks.layers
        for i, layer in enumerate(layers):
            layer.load_state_dict(synthetic_layer_state_dict(mc, seed=seed * 1000 + i, device=dev, fp8=fp8 and 0 < i < len(layers) - 1))

    # ---- pieces of get_embedding_and_meta ---------------------------------------------------------------------------------------
    def _timestep_embedding(self, t: torch.Tensor) -> torch.Tensor:
        """TimestepEmbedder.forward (dit_module.py:76-106): cos | sin of t * 1000 * 10000^(-i/half), rounded to the parameter dtype,
        then Linear -> SiLU -> Linear in fp32."""
        half = self.frequency_embedding_size // 2
        freqs = self._t_freqs                                      # made once per model (and device); read-only
        if freqs is None or freqs.device != t.device:
            freqs = self._t_freqs = torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=torch.float32, device=t.device) / half)
        args = t[:, None].float() * freqs[None] * 1000.0
        tf = torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(BF16).float()
        w = self.w
        return F.linear(F.silu(F.linear(tf, w["t_embedder.mlp.0.weight"], w["t_embedder.mlp.0.bias"])),
                        w["t_embedder.mlp.2.weight"], w["t_embedder.mlp.2.bias"])

    def _rope(self, t_total: int, H: int, W: int, rows: int) -> torch.Tensor:
        """LearnableRotaryEmbeddingCat.get_embed (dit_module.py:602-776, in_pixels=False) for [t_total, H, W] with the reference
        shape [t_total, H / r, W / r], r = sqrt(H W / 256) (dit_model.py:157-166); the last `rows` rows (sin | cos).  Memoised per
        argument tuple and device: two forwards of one geometry get the SAME tensor, which nobody may write."""
        return _memoised(self._rope_memo, (t_total, H, W, rows, str(self.device)), lambda: self._build_rope(t_total, H, W, rows))

    def _build_rope(self, t_total: int, H: int, W: int, rows: int) -> torch.Tensor:
        dev, bands = self.device, self.w["rope.bands"]
        r = math.sqrt((H * W) / (16 * 16))
        shape, ref = [t_total, H, W], [t_total, H / r, W / r]
        axes = [torch.arange(s, dtype=torch.int64, device=dev).to(torch.float32) for s in shape]
        axes[1] = axes[1] - (H - 1) / 2
        axes[2] = axes[2] - (W - 1) / 2
        scaled = [a if f == 1 else a / (f - 1) * (rf - 1) for a, f, rf in zip(axes, shape, ref)]
        grid = torch.stack(torch.meshgrid(*scaled, indexing="ij"), dim=-1).unsqueeze(-1)
        pos = grid * bands
        n = t_total * H * W
        return torch.cat([pos.sin().reshape(n, -1), pos.cos().reshape(n, -1)], -1)[-rows:].contiguous()

    def _packed_ranges(self, lengths) -> Tuple[torch.Tensor, torch.Tensor, np.ndarray]:
        """Packed segments of the given lengths: `(cu_seqlens int32 [n + 1], ranges int32 [n, 2])` on the device — built on the host and
        sent through pinned memory — and the ranges' host copy.  Memoised by the caller: read-only."""
        cu = cu_seqlens(lengths)
        ranges = np.stack([cu[:-1], cu[1:]], axis=1)
        return _upload(cu, self.device), _upload(ranges, self.device), ranges

    def forward_pre_process(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None, **kwargs
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, ModelMetaArgs]:
        assert kv_range is not None, "Please ensure kv_range is provided"
        if caption_dropout_mask is None:
            raise ValueError("caption_dropout_mask is required at inference: the AdaLN branch of the caption embedder reads the learned "
                             "null caption it selects (dit_module.py:141-160)")
        assert xattn_mask is not None
        dev, w = self.device, self.w
        plan: Optional[RangePlan] = kwargs.get("range_plan")
        x, t, y = x.to(dev), t.to(dev).float(), y.to(dev).float()
        if self.half_channel_vae:
            assert x.shape[1] == 16
        # Part 1: patch embedding (a Conv3d whose stride equals its kernel)
        # stride == kernel: the convolution is one [tokens, C pT pH pW] x [C pT pH pW, hidden] product (MIOpen's fp32 Conv3d for this
        # shape is a naive direct kernel: 6 ms per call at 720 x 720, as long as four of the 34 layers)
        pt, pp = self.t_patch_size, self.patch_size
        N, _, Tf, Hf, Wf = x.shape
        T, H, Wd = Tf // pt, Hf // pp, Wf // pp
        if x.is_cuda and x.dtype in (torch.float32, BF16):
            # x * x_rescale_factor (in x's dtype), the half_channel_vae copy, .float() and the "(C pT pH pW)" gather of every patch:
            # one launch, bit for bit the torch chain below
            cols = ops.magi_patch_rows(x if x.stride(-1) == 1 else x.contiguous(), (pt, pp, pp), self.x_rescale_factor, self.half_channel_vae)
        else:       # a model built on the CPU (the host side alone, for checks without a GPU), or a dtype the kernel does not read
            x = x * self.x_rescale_factor
            x = (torch.cat([x, x], dim=1) if self.half_channel_vae else x).float()
            C = x.shape[1]
            cols = x[:, :, :T * pt, :H * pp, :Wd * pp].reshape(N, C, T, pt, H, pp, Wd, pp).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(N, T * H * Wd, -1)
        xe = F.linear(cols, w["x_embedder.weight"].reshape(w["x_embedder.weight"].shape[0], -1))      # [N, (T H W), hidden]
        range_num, dn = kwargs["range_num"], kwargs["denoising_range_num"]
        slice_point = kwargs.get("slice_point", 0)
        frame_in_range = T // dn
        # Part 2: rope
        rope = self._rope(T + frame_in_range * slice_point, H, Wd, T * H * Wd)
        # Part 3: timestep embedding
        assert t.shape[0] == N and t.shape[1] == dn, f"Invalid t shape {tuple(t.shape)}"
        te = self._timestep_embedding(t.flatten())
        if _cfg(self.engine_config, "distill", False):
            if kwargs["num_steps"] == 12:
                factor = 4 / kwargs["distill_interval"] * 2
            else:
                factor = kwargs["num_steps"] / 4 * 2
            te = te + self._timestep_embedding(torch.ones_like(t.flatten()) * factor)
        te = te.reshape(N, dn, -1)
        # Part 4: caption: cross-attention rows from the caption itself, the AdaLN row from the learned null caption
        y_xattn = F.silu(F.linear(y, w["y_embedder.y_proj_xattn.0.weight"], w["y_embedder.y_proj_xattn.0.bias"]))
        null = w["y_embedder.null_caption_embedding"]
        drop = caption_dropout_mask.to(dev).bool()
        cap = torch.where(drop[:, None, None], null[None, -1, :], null[None, -2, :])
        y_adaln = F.linear(cap, w["y_embedder.y_proj_adaln.0.weight"], w["y_embedder.y_proj_adaln.0.bias"]).squeeze(1)
        mask = xattn_mask.to(dev).squeeze(1).squeeze(1)
        condition = te + y_adaln.unsqueeze(1)
        assert condition.shape[0] == N and condition.shape[1] == dn
        per = (T * H * Wd) // dn
        condition_map = _memoised(self._map_memo, (N, dn, per, str(dev)), lambda: torch.repeat_interleave(
            torch.arange(N * dn, device=dev), per).reshape(N, -1).transpose(0, 1).contiguous())            # shared between forwards: read-only
        clip = H * Wd * frame_in_range
        kv_range = kv_range.to(dev)
        y_rows = y_xattn.squeeze(1)
        if plan is None:
            # the caller handed over device tensors only: the packed ranges are read back from them, each read a wait for the device
            y_flat = torch.masked_select(y_rows, mask.unsqueeze(-1).bool()).reshape(-1, y_xattn.shape[-1])
            # Part 5 / 6: packed ranges
            y_index = mask.reshape(mask.shape[0], -1).sum(-1)
            cu_q = torch.tensor([0] + [clip] * dn * N, device=dev).cumsum(-1).to(torch.int32)
            cu_k = torch.cat([y_index.new_zeros(1), y_index]).to(torch.int64).cumsum(-1).to(torch.int32)
            q_ranges = torch.stack([cu_q[:-1], cu_q[1:]], 1)
            k_ranges_x = torch.stack([cu_k[:-1], cu_k[1:]], 1)
            cross = PackedCrossAttnParams(q_ranges=q_ranges, kv_ranges=k_ranges_x, cu_seqlens_q=cu_q, cu_seqlens_kv=cu_k,
                                          max_seqlen_q=clip, max_seqlen_kv=self.caption_max_length)
            flat_kv = torch.unique(kv_range, sorted=True)
            max_seqlen_k = int((flat_kv[-1] - flat_kv[0]).item())
            np_q_range, np_k_range = q_ranges.cpu().numpy(), kv_range.cpu().numpy()
        else:
            # the same tensors from what the host knows (RangePlan): nothing below reads the device or uploads from pageable memory
            lens = plan.caption_lens
            if len(lens) != y_rows.shape[0] or plan.kv_range.shape[0] != kv_range.shape[0] or max(lens, default=0) > y_rows.shape[1]:
                raise ValueError(f"range_plan describes {len(lens)} caption rows (longest {max(lens, default=0)}) and {plan.kv_range.shape[0]} "
                                 f"key ranges, the forward has {y_rows.shape[0]} rows of {y_rows.shape[1]} and {kv_range.shape[0]} ranges")
            if all(n == y_rows.shape[1] for n in lens):
                y_flat = y_rows.reshape(-1, y_rows.shape[-1])
            else:                                                  # masked_select's rows: the first lens[i] tokens of caption i, in order
                y_flat = torch.cat([y_rows[i, :n] for i, n in enumerate(lens)], dim=0)
            cu_q, q_ranges, np_q_range = _memoised(self._range_memo, ("q", dn * N, clip, str(dev)), lambda: self._packed_ranges([clip] * (dn * N)))
            cu_k, k_ranges_x, host_k = _memoised(self._range_memo, ("k", lens, str(dev)), lambda: self._packed_ranges(lens))
            cross = PackedCrossAttnParams(q_ranges=q_ranges, kv_ranges=k_ranges_x, cu_seqlens_q=cu_q, cu_seqlens_kv=cu_k,
                                          max_seqlen_q=clip, max_seqlen_kv=self.caption_max_length,
                                          host_q_ranges=np_q_range.tolist(), host_kv_ranges=host_k.tolist())
            max_seqlen_k, np_k_range = plan.max_seqlen_k, plan.kv_range
        ardf = dict(clip_token_nums=clip, slice_point=slice_point, range_num=range_num, denoising_range_num=dn, q_range=q_ranges,
                    k_range=kv_range, max_seqlen_q=clip, max_seqlen_k=max_seqlen_k)
        xs = xe.to(BF16).transpose(0, 1).contiguous()                                              # "N C T H W -> (T H W) N C"
        core = PackedCoreAttnParams(q_range=ardf["q_range"], k_range=ardf["k_range"], np_q_range=np_q_range,
                                    np_k_range=np_k_range, max_seqlen_q=clip, max_seqlen_k=ardf["max_seqlen_k"])
        ec = self.engine_config
        xs, condition_map, rope, pad, sizes, core, cross = cpl.cp_pre_process(
            _cfg(ec, "cp_size", 1), _cfg(ec, "cp_strategy", "none"), xs, condition_map, rope, None, ardf, core, cross)
        meta = ModelMetaArgs(H=H, W=Wd, cp_pad_size=pad, cp_split_sizes=sizes, slice_point=slice_point, denoising_range_num=dn,
                             range_num=range_num, extract_prefix_video_feature=kwargs.get("extract_prefix_video_feature", False),
                             fwd_extra_1st_chunk=kwargs["fwd_extra_1st_chunk"],
                             distill_nearly_clean_chunk=kwargs.get("distill_nearly_clean_chunk", False), clip_token_nums=clip,
                             enable_cuda_graph=False, core_attn_params=core, cross_attn_params=cross)
        return xs, condition.to(BF16), condition_map, y_flat.to(BF16), rope, meta

    def forward_post_process(self, hidden: torch.Tensor, meta: ModelMetaArgs) -> torch.Tensor:
        mc, w = self.model_config, self.w
        gamma = w["videodit_blocks.final_layernorm.weight"]
        gamma = gamma + 1 if bool(_cfg(mc, "apply_layernorm_1p", False)) else gamma
        hn = F.layer_norm(hidden.float(), (hidden.shape[-1],), gamma, w["videodit_blocks.final_layernorm.bias"], mc.layernorm_epsilon)
        o = F.linear(hn, w["final_linear.linear.weight"])                                        # (thw / cp, N, pT pH pW C)
        ec = self.engine_config
        o = cpl.cp_post_process(_cfg(ec, "cp_size", 1), _cfg(ec, "cp_strategy", "none"), o, meta)
        S, N, K = o.shape
        pt, p, C = self.t_patch_size, self.patch_size, self.out_channels
        H, Wd = meta.H, meta.W
        T = S // (H * Wd)
        assert S == T * H * Wd and K == pt * p * p * C, (tuple(o.shape), (T, H, Wd), (pt, p, p, C))
        if self.half_channel_vae:
            assert C == 32
        # "(T H W) N (pT pH pW C) -> N C (T pT) (H pH) (W pW)", the first 16 channels of a half_channel_vae model, / x_rescale_factor:
        # one launch, bit for bit the torch chain below (reshape, 8-D permute, contiguous, slice, true divide)
        if o.is_cuda:
            return ops.magi_unpatch(o, (T, H, Wd), (pt, p, p), self.x_rescale_factor, 16 if self.half_channel_vae else None)
        o = o.reshape(T, H, Wd, N, pt, p, p, C).permute(3, 7, 0, 4, 1, 5, 2, 6).reshape(N, C, T * pt, H * p, Wd * p).contiguous()      # a CPU model
        if self.half_channel_vae:
            o = o[:, :16]
        return o / self.x_rescale_factor

    @torch.no_grad()
    def forward(self, x, t, y, caption_dropout_mask=None, xattn_mask=None, kv_range=None,
                inference_params: Optional[InferenceParams] = None, **kwargs) -> torch.Tensor:
        if x.shape[0] > 1:
            # a batch: only the unconditional pass of forward_3cfg has one (chunks turned into batch rows, no cache, dit_model.py:436-489).
            # The layers run the cached path with batch 1; rows of a batch do not interact, so they go through one at a time — row b with
            # its own timesteps, its captions (range_num = denoising ranges per row) and its key ranges rebased to the row.
            if inference_params is not None:
                raise NotImplementedError("HipVideoDiTModel.forward: a batch with a KV cache (the reference batches only forward_3cfg's "
                                          "unconditional pass, inference_params=None)")
            N, dn = x.shape[0], kwargs["denoising_range_num"]
            rows = kv_range.shape[0] // N
            drop = caption_dropout_mask.expand(N) if caption_dropout_mask.numel() == 1 else caption_dropout_mask
            outs = []
            plan = kwargs.get("range_plan")
            for b in range(N):
                kv = kv_range[b * rows:(b + 1) * rows]
                kw = kwargs if plan is None else dict(kwargs, range_plan=plan.batch_row(b, N, dn))      # rebased as the tensor is
                outs.append(self.forward(x[b:b + 1], t[b:b + 1], y[b * dn:(b + 1) * dn], drop[b:b + 1], xattn_mask[b * dn:(b + 1) * dn],
                                         kv - kv.min(), None, **kw))
            return torch.cat(outs, dim=0)
        xs, condition, condition_map, y_flat, rope, meta = self.forward_pre_process(x, t, y, caption_dropout_mask, xattn_mask, kv_range, **kwargs)
        hs = self.videodit_blocks(xs.clone(), condition, condition_map, y_flat, rope, inference_params, meta)
        return self.forward_post_process(hs, meta)

    __call__ = forward

    @torch.no_grad()
    def forward_3cfg(self, x, timestep, y, mask, kv_range, inference_params, **kwargs):
        """dit_model.py:399-492: the three forwards of classifier-free guidance — (previous chunks + text) WITHOUT touching the cache,
        (previous chunks, null caption) which writes it, and the unconditional one: the denoising chunks as batch rows that see only
        themselves, no cache.  -> (out_cond_pre_and_text, out_cond_pre, out_uncond, denoise_width)."""
        assert x.shape[0] == 2 and mask.shape[0] % 2 == 0
        x = torch.cat([x[0:1], x[0:1]], dim=0)
        half = y.shape[0] // 2
        drop = torch.arange(2, device=x.device) > 0               # [False, True], made on the device: no blocking upload per step
        kwargs = dict(kwargs)
        # a RangePlan describes the call's key ranges and all its caption rows; each of the three forwards gets the plan of its own rows
        plan: Optional[RangePlan] = kwargs.pop("range_plan", None)
        inference_params.update_kv_cache = False
        out_text = self.forward(x[0:1], timestep[0:1], y[0:half], caption_dropout_mask=drop[0:1], xattn_mask=mask[0:half],
                                kv_range=kv_range, inference_params=inference_params, **kwargs,
                                **_with_plan(plan and plan.captions(0, half)))
        inference_params.update_kv_cache = True
        out_pre = self.forward(x[1:2], timestep[1:2], y[half:], caption_dropout_mask=drop[1:2], xattn_mask=mask[half:],
                               kv_range=kv_range, inference_params=inference_params, **kwargs,
                               **_with_plan(plan and plan.captions(half, None)))
        cw = kwargs["chunk_width"]
        dn = kwargs["denoising_range_num"] - (1 if kwargs.get("fwd_extra_1st_chunk", False) else 0)     # UnconditionGuard (:448-469)
        denoise_width = cw * dn
        u = x[0:1, :, -denoise_width:].squeeze(0)
        uncond_x = u.reshape(-1, dn, cw, *u.shape[2:]).transpose(0, 1)                                   # chunk_to_batch: [dn, C, cw, H, W]
        ukw = dict(kwargs, range_num=1, denoising_range_num=1, slice_point=0, fwd_extra_1st_chunk=False)
        if plan is not None:
            ukw["range_plan"] = RangePlan.uncondition(dn, _row_tokens(self, uncond_x), plan.caption_lens[half:][-dn:])
        out_uncond = self.forward(uncond_x, timestep[0:1, -dn:].transpose(0, 1), y[half:][-dn:],
                                  caption_dropout_mask=torch.ones(1, dtype=torch.bool, device=x.device), xattn_mask=mask[half:][-dn:],
                                  kv_range=self.generate_kv_range_for_uncondition(uncond_x), inference_params=None, **ukw)
        o = out_uncond.transpose(0, 1)
        out_uncond = o.reshape(1, -1, dn * cw, *o.shape[3:])                                             # batch_to_chunk
        return out_text, out_pre, out_uncond, denoise_width

    def _dispatch_3cfg(self, x, timestep, y, mask, kv_range, inference_params, **kwargs) -> torch.Tensor:
        """dit_model.py:500-535: per denoising chunk, scales looked up by its timestep in `cfg_t_range`:
        (1 - s_prev) uncond + (s_prev - s_text) cond_pre + s_text cond_pre_and_text."""
        rc = self.runtime_config
        out_text, out_pre, out_uncond, denoise_width = self.forward_3cfg(x, timestep, y, mask, kv_range, inference_params, **kwargs)
        dev = out_text.device
        # the three guidance tables go up once per model (and per value: a changed runtime_config makes new ones), not once per call
        key = (tuple(rc.prev_chunk_scales), tuple(rc.text_scales), tuple(rc.cfg_t_range), str(dev))
        memo = getattr(self, "_guidance_memo", None)
        if memo is None or memo[0] != key:
            up = (lambda t: t.pin_memory().to(dev, non_blocking=True)) if dev.type == "cuda" else (lambda t: t)
            memo = self._guidance_memo = (key, tuple(up(torch.tensor(v)) for v in (rc.prev_chunk_scales, rc.text_scales, rc.cfg_t_range)))
        prev_s, text_s, t_range = memo[1]                          # read-only
        assert len(prev_s) == len(t_range) and len(text_s) == len(t_range), "prev_chunk_scales / text_scales and cfg_t_range differ in length"
        planned = kwargs.get("range_plan") is not None             # the caller keeps the host free: it has checked the timesteps' bins itself
        n, cw = kwargs["denoising_range_num"], kwargs["chunk_width"]
        if kwargs["fwd_extra_1st_chunk"]:
            n -= 1
        cfg_t = timestep[0, -n:].to(dev)
        pieces = []
        for ci in range(n):
            idx = torch.searchsorted(t_range - 1e-7, cfg_t[ci]) - 1                                       # get_cfg_scale (:494-497)
            if planned:                                            # a gather on the device (a one-element index), not a read of idx
                sp, st = prev_s[idx.reshape(1)], text_s[idx.reshape(1)]
            else:
                assert 0 <= int(idx) < len(prev_s)
                sp, st = prev_s[idx], text_s[idx]
            sl = slice(ci * cw, (ci + 1) * cw)
            pieces.append((1 - sp) * out_uncond[:, :, sl] + (sp - st) * out_pre[:, :, -denoise_width:][:, :, sl]
                          + st * out_text[:, :, -denoise_width:][:, :, sl])
        x = torch.cat([x[0:1, :, :-denoise_width].to(dev), torch.cat(pieces, dim=2)], dim=2)
        return torch.cat([x, x], dim=0)

    @torch.no_grad()
    def forward_velocities(self, x, timestep, y, mask, kv_range, inference_params, *, nearly_clean: bool = False, cfg_bins=None,
                           **kwargs):
        """The forwards of `forward_dispatcher` WITHOUT its mixing: the raw outputs and where they lie, as the source list of
        `hip_ops.magi_integrate` — `[(v, first_frame, first_chunk, last_chunk, weights), ...]`, chunks counted inside the window of
        denoising chunks (the clean chunk in front is not one of them).  What the dispatcher reads off the device is handed in
        instead: `nearly_clean` (the decision `distill_nearly_clean_chunk`) and, for `cfg_number == 3`, `cfg_bins`, the bin of
        `cfg_t_range` of every denoising chunk (`schedule.cfg_bins`).
          cfg_number == 1: one source, weight 1; nearly clean: the widened forward's output twice — its frames from the first
                           denoising chunk on, and the re-forwarded copy at frame `width` on window chunk 0 — at `scale` / `1 - scale`
          cfg_number == 3: `out_uncond` from frame 0, `out_pre` and `out_text` from `-denoise_width`, at `(1 - s_prev)`,
                           `(s_prev - s_text)`, `s_text`."""
        import os
        from . import schedule as sched
        rc = self.runtime_config
        cfg_number = getattr(rc, "cfg_number", None)
        if cfg_number not in (1, 3):
            raise NotImplementedError("HipVideoDiTModel.forward_velocities: runtime_config.cfg_number must be 1 (distilled checkpoints) or 3 "
                                      "(the reference's own NotImplementedError for anything else, dit_model.py:596)")
        kwargs = dict(kwargs, distill_nearly_clean_chunk=bool(nearly_clean))
        cw, extra = kwargs["chunk_width"], bool(kwargs["fwd_extra_1st_chunk"])
        n = kwargs["denoising_range_num"] - int(extra)
        if cfg_number == 3:
            if cfg_bins is None or len(cfg_bins) != n:
                raise ValueError(f"forward_velocities: cfg_number 3 needs one cfg_t_range bin per denoising chunk ({n}), got {cfg_bins}")
            assert len(rc.prev_chunk_scales) == len(rc.cfg_t_range) and len(rc.text_scales) == len(rc.cfg_t_range), \
                "prev_chunk_scales / text_scales and cfg_t_range differ in length"
            out_text, out_pre, out_uncond, denoise_width = self.forward_3cfg(x, timestep, y, mask, kv_range, inference_params, **kwargs)
            w_uncond, w_pre, w_text = sched.cfg_weights(cfg_bins, rc.prev_chunk_scales, rc.text_scales)
            return [(out_uncond, 0, 0, n - 1, w_uncond), (out_pre, -denoise_width, 0, n - 1, w_pre),
                    (out_text, -denoise_width, 0, n - 1, w_text)]
        assert x.shape[0] == 2
        kwargs["caption_dropout_mask"] = torch.zeros(1, dtype=torch.bool, device=x.device)
        inference_params.update_kv_cache = True
        half = y.shape[0] // 2
        s0 = 1 if extra else 0
        plan: Optional[RangePlan] = kwargs.pop("range_plan", None)          # of the whole call: every caption row, the conditional half first
        if nearly_clean:
            scale, rest = sched.nearly_clean_weights(float(os.getenv("prev_chunks_scale", 0.7)))
            width = x.shape[2]
            new_x = x[0:1, :, s0 * cw:(s0 + 1) * cw]
            new_kv = self.generate_kv_range_for_uncondition(new_x) + kv_range.max()
            kwargs["denoising_range_num"] += 1
            out = self.forward(torch.cat([x[0:1], new_x], dim=2), torch.cat([timestep[0:1], timestep[0:1, s0:s0 + 1]], dim=1),
                               torch.cat([y[0:half], y[s0:s0 + 1]], dim=0), xattn_mask=torch.cat([mask[0:half], mask[s0:s0 + 1]], dim=0),
                               kv_range=torch.cat([kv_range.to(new_kv.device), new_kv], dim=0), inference_params=inference_params, **kwargs,
                               **_with_plan(plan and plan.extended(_row_tokens(self, new_x), s0, half)))
            return [(out, s0 * cw, 0, n - 1, [scale] + [1.0] * (n - 1)), (out, width, 0, 0, [rest] + [0.0] * (n - 1))]
        out = self.forward(x[0:1], timestep[0:1], y[0:half], xattn_mask=mask[0:half], kv_range=kv_range,
                           inference_params=inference_params, **kwargs, **_with_plan(plan and plan.captions(0, half)))
        return [(out, s0 * cw, 0, n - 1, [1.0] * n)]

    def generate_kv_range_for_uncondition(self, uncond_x: torch.Tensor) -> torch.Tensor:
        """dit_model.py:91-100: one self-contained key range per batch row of `uncond_x`, `[[b n, (b + 1) n] for b in range(B)]` int32,
        formed on the device (a host list would be a blocking upload in every guidance and nearly-clean step)."""
        B, _, T, H, W = uncond_x.shape
        n = (T // self.t_patch_size) * (H // self.patch_size) * (W // self.patch_size)
        b = torch.arange(B, dtype=torch.int32, device=self.device)
        return torch.stack([b * n, (b + 1) * n], dim=1)

    @torch.no_grad()
    def forward_dispatcher(self, x, timestep, y, mask, kv_range, inference_params, **kwargs) -> torch.Tensor:
        """dit_model.py:499-596 for `runtime_config.cfg_number == 1` (the distilled checkpoints: one conditional forward, no guidance
        batch).  x `[2, C, T, H, W]` with equal halves, y / mask hold the conditional rows first.  When the newest finished chunk is
        nearly clean (`distill_nearly_clean_chunk`) it is forwarded a second time as an extra range that sees only itself, and the two
        results are blended `prev_chunks_scale : 1 - prev_chunks_scale` (env `prev_chunks_scale`, 0.7)."""
        import os
        rc = self.runtime_config
        if rc is not None and getattr(rc, "cfg_number", None) == 3:
            return self._dispatch_3cfg(x, timestep, y, mask, kv_range, inference_params, **kwargs)
        if rc is None or getattr(rc, "cfg_number", None) != 1:
            raise NotImplementedError("HipVideoDiTModel.forward_dispatcher: runtime_config.cfg_number must be 1 (distilled checkpoints) or 3 "
                                      "(the reference's own NotImplementedError for anything else, dit_model.py:596)")
        assert x.shape[0] == 2
        x = torch.cat([x[0:1], x[0:1]], dim=0)
        kwargs = dict(kwargs)
        kwargs["caption_dropout_mask"] = torch.zeros(1, dtype=torch.bool, device=x.device)       # [False], made on the device: no upload
        inference_params.update_kv_cache = True
        half = y.shape[0] // 2
        cw = kwargs["chunk_width"]
        plan: Optional[RangePlan] = kwargs.pop("range_plan", None)
        if kwargs.get("distill_nearly_clean_chunk", False):
            scale = float(os.getenv("prev_chunks_scale", 0.7))
            s0 = 1 if kwargs["fwd_extra_1st_chunk"] else 0
            width = x.shape[2]
            new_x = x[0:1, :, s0 * cw:(s0 + 1) * cw]
            new_kv = self.generate_kv_range_for_uncondition(new_x) + kv_range.max()
            kwargs["denoising_range_num"] += 1
            out = self.forward(torch.cat([x[0:1], new_x], dim=2), torch.cat([timestep[0:1], timestep[0:1, s0:s0 + 1]], dim=1),
                               torch.cat([y[0:half], y[s0:s0 + 1]], dim=0), xattn_mask=torch.cat([mask[0:half], mask[s0:s0 + 1]], dim=0),
                               kv_range=torch.cat([kv_range.to(new_kv.device), new_kv], dim=0), inference_params=inference_params, **kwargs,
                               **_with_plan(plan and plan.extended(_row_tokens(self, new_x), s0, half)))
            out[:, :, s0 * cw:(s0 + 1) * cw] = out[:, :, s0 * cw:(s0 + 1) * cw] * scale + out[:, :, width:] * (1 - scale)
            out = out[:, :, :width]
        else:
            out = self.forward(x[0:1], timestep[0:1], y[0:half], xattn_mask=mask[0:half], kv_range=kv_range,
                               inference_params=inference_params, **kwargs, **_with_plan(plan and plan.captions(0, half)))
        denoise_width = cw * kwargs["denoising_range_num"]
        if kwargs["fwd_extra_1st_chunk"]:
            denoise_width -= cw
        x = torch.cat([x[0:1, :, :-denoise_width], out[:, :, -denoise_width:]], dim=2)
        return torch.cat([x[0:1], x[0:1]], dim=0)

"""MAGI-1 ViT-VAE tile decoder on MI355X: one latent tile -> pixels (BASELINE config 5, PER_BLOCK decode).

Mirrors `inferix/models/magi/vae/vae_module.py` / `vae_model.py` of the reference:
  ViTDecoder.forward        vae_module.py:676-716   proj_in, class token, positional embedding, the blocks, final norm,
                                                    final_proj + final_norm, un-patching + last-layer convolution
  Block / Attention / Mlp   :207-346                per block: (LayerNorm unless ln_in_attn) -> qkv GEMM -> ifx_vit_head_prep ->
                                                    ifx_vit_attention -> proj GEMM + residual -> LayerNorm -> fc1 GEMM + exact GELU ->
                                                    fc2 GEMM + residual
  resize_pos_embed          :400-406                host-side torch, once per latent shape, cached
  ViTVAE.decode             vae_model.py:290-308    the T == 1 rule

Every launch goes through inferix_amd.hip_ops; what is left to torch on the device is the token bookkeeping of the embedding (zero
padding of the z_chans input columns to one GEMM K-step, the proj_in bias, the class-token row, the bf16 addition of the positional
table).

Not here: `use_rope=True` — the reference's own rotary path raises on every input (the [1, N - 1, 1, cols] tables broadcast against
the 5-D q slice, :289-291, and carry 6 * (head_dim // 6) columns, :182-201), so there is no result to reproduce; the rotation of
ifx_vit_head_prep is available to a caller with tables of its own.  Head sizes other than 64 and un-patch widths other than 4 channels
are not built.  The encoder and checkpoint download stay with the caller.

The chunk decode around the tiles (`ViTVAE.tiled_decode_3d` vae_model.py:179-219, `TileProcessor.tiled_decode`
distributed/parallelism/tile_parallel.py:348-448, `VaeHelper.decode` pipeline/magi/video_process.py:155-200) is
`HipMagiVAEDecoder.tiled_decode_3d`: the tiles of a chunk are grouped by latent shape (magi/tiles.py), every group is one batched decoder
forward whose last kernel writes into one arena, and one ifx_vit_tile_blend launch blends, crops, concatenates and converts.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import _hip
from .. import hip_ops as ops
from . import tiles as _tiles

BF16 = torch.bfloat16
LN_EPS = 1e-5      # nn.LayerNorm's default and ManualLayerNorm's eps
MAX_ROWS_PER_FORWARD = 65536       # token rows per batched decoder forward: the 18 x 3073 = 55314 rows of config 5's largest group fit


class HipViTDecoder:
    """`ViTDecoder(**ddconfig)` with `.forward(x: [B, z_chans, lT, lH, lW]) -> [B, 3, lT pT, lH pH, lW pW]` (bf16, on the device) and the
    reference's state-dict keys: `proj_in`, `cls_token`, `pos_embed`, `blocks.N.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}`,
    `norm`, `final_proj`, `final_norm`, `last_layer`."""

    def __init__(self, video_size=256, video_length=16, patch_size=8, patch_length=4, in_chans=3, z_chans=4, double_z=True, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=None, with_cls_token=True, norm_code=False, ln_in_attn=False, conv_last_layer=False,
                 use_rope=False, use_final_proj=False, device="cuda"):
        assert conv_last_layer is True, "Only support conv_last_layer=True"           # as upstream (:643)
        if norm_layer is not None and norm_layer is not torch.nn.LayerNorm:
            raise NotImplementedError("HipViTDecoder: norm_layer other than nn.LayerNorm")
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f"HipViTDecoder: head size {embed_dim / num_heads:g} (ifx_vit_attention is built for 64)")
        if use_rope:
            raise NotImplementedError("HipViTDecoder: use_rope=True raises in the reference's own forward (vae_module.py:289-291 broadcasts "
                                      "the tables against a 5-D slice); there is no result to reproduce")
        if qk_scale is not None:
            raise NotImplementedError("HipViTDecoder: qk_scale (the reference's Attention ignores it too)")
        self.device = torch.device(device)
        self.embed_dim, self.depth, self.num_heads, self.z_chans = embed_dim, depth, num_heads, z_chans
        self.patch_size, self.patch_length = patch_size, patch_length
        self.latent_size, self.latent_length = video_size // patch_size, video_length // patch_length
        self.hidden = int(embed_dim * mlp_ratio)
        self.qkv_bias, self.ln_in_attn, self.use_final_proj, self.with_cls_token = qkv_bias, ln_in_attn, use_final_proj, with_cls_token
        self.cls_token_nums = 1 if with_cls_token else 0
        patch_volume = patch_size * patch_size * patch_length
        self.unpatch_channels = 4 if use_final_proj else embed_dim // patch_volume
        if self.unpatch_channels != 4 or (not use_final_proj and embed_dim != 4 * patch_volume):
            raise NotImplementedError(f"HipViTDecoder: {embed_dim} / {patch_volume} un-patch channels (ifx_vit_unpatch_conv is built for 4)")
        self.w: Dict[str, torch.Tensor] = {}
        self._proj_in_padded: Optional[torch.Tensor] = None
        self._pos_embed_host: Optional[torch.Tensor] = None
        self._pos_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def _expected(self) -> Dict[str, Tuple[int, ...]]:
        D, hid = self.embed_dim, self.hidden
        n_pos = self.latent_length * self.latent_size * self.latent_size + self.cls_token_nums
        s = {"proj_in.weight": (D, self.z_chans), "proj_in.bias": (D,), "pos_embed": (1, n_pos, D), "norm.weight": (D,), "norm.bias": (D,),
             "last_layer.weight": (3, 4, 3, 3, 3), "last_layer.bias": (3,)}
        if self.with_cls_token:
            s["cls_token"] = (1, 1, D)
        for i in range(self.depth):
            p = f"blocks.{i}."
            if not self.ln_in_attn:
                s[p + "norm1.weight"], s[p + "norm1.bias"] = (D,), (D,)
            s[p + "attn.qkv.weight"] = (3 * D, D)
            if self.qkv_bias:
                s[p + "attn.qkv.bias"] = (3 * D,)
            s[p + "attn.proj.weight"], s[p + "attn.proj.bias"] = (D, D), (D,)
            s[p + "norm2.weight"], s[p + "norm2.bias"] = (D,), (D,)
            s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (hid, D), (hid,)
            s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (D, hid), (D,)
        if self.use_final_proj:
            n = 4 * self.patch_size * self.patch_size * self.patch_length
            s["final_proj.weight"], s["final_proj.bias"] = (n, D), (n,)
            s["final_norm.weight"], s["final_norm.bias"] = (n,), (n,)
        return s

    def load_state_dict(self, W: Dict[str, torch.Tensor], prefix: str = "") -> None:
        w = {}
        for k, shape in self._expected().items():
            if prefix + k not in W:
                raise KeyError(f"HipViTDecoder.load_state_dict: missing {prefix + k}")
            t = W[prefix + k]
            if tuple(t.shape) != shape:
                raise ValueError(f"HipViTDecoder.load_state_dict: {prefix + k} has shape {tuple(t.shape)}, expected {shape}")
            w[k] = t.detach().to(self.device, BF16).contiguous()
        self.w = w
        pad = torch.zeros(self.embed_dim, 64, dtype=BF16, device=self.device)        # K = z_chans padded to one 64-wide GEMM K-step
        pad[:, :self.z_chans] = w["proj_in.weight"]
        self._proj_in_padded = pad
        self._pos_embed_host = w["pos_embed"].cpu()
        self._pos_cache = {}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return dict(self.w)

    def load_synthetic(self, seed: int = 0) -> None:
        """Random weights with the reference's shapes, generated on the device (benchmarks; no checkpoint exists offline)."""
        g = torch.Generator(device=self.device).manual_seed(seed)
        W = {}
        for k, shape in self._expected().items():
            t = torch.randn(*shape, generator=g, device=self.device)
            if k.endswith(".weight") and len(shape) > 1:
                t = t * (t[0].numel() ** -0.5)
            elif k.endswith(".weight"):
                t = 1.0 + 0.1 * t
            elif k.endswith(".bias"):
                t = 0.05 * t
            else:
                t = 0.5 * t
            W[k] = t.to(BF16)
        self.load_state_dict(W)

    # ---- host-side tables -----------------------------------------------------------------------------------------------------------
    def _pos_embed(self, latent: Tuple[int, int, int]) -> torch.Tensor:
        """`[cls + tokens, D]` on the device for this latent shape: the trained table, or its patch rows resampled as a volume
        (trilinear, align_corners off, bf16 on the host as the module's parameter is) behind the untouched class row."""
        pe = self._pos_cache.get(latent)
        if pe is None:
            trained = (self.latent_length, self.latent_size, self.latent_size)
            pe = self._pos_embed_host
            if latent != trained:
                if not self.with_cls_token:
                    raise NotImplementedError("HipViTDecoder: the reference's resize drops row 0 of pos_embed, it needs the class token")
                D = self.embed_dim
                vol = pe[:, 1:, :].reshape(1, *trained, D).permute(0, 4, 1, 2, 3)
                vol = F.interpolate(vol, size=latent, mode="trilinear", align_corners=False)
                pe = torch.cat((pe[:, 0:1, :], vol.permute(0, 2, 3, 4, 1).reshape(1, -1, D)), dim=1)
            pe = self._pos_cache[latent] = pe[0].to(self.device).contiguous()
        return pe

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def embed(self, x: torch.Tensor) -> torch.Tensor:
        """:677-699 -> token rows `[B, cls + tokens, D]`."""
        if not x.is_cuda:
            raise _hip.HipKernelError(f"HipViTDecoder: input is on {x.device}; inferix_amd runs on the GPU only")
        if not self.w:
            raise RuntimeError("HipViTDecoder: no weights loaded")
        B, C, lt, lh, lw = x.shape
        assert C == self.z_chans, (C, self.z_chans)
        rows = torch.zeros(B * lt * lh * lw, 64, dtype=BF16, device=x.device)
        rows[:, :C] = x.to(BF16).permute(0, 2, 3, 4, 1).reshape(-1, C)
        # the bias is added to the ROUNDED product: that is how torch's CPU linear evaluates this K = z_chans projection on a 3-D input
        # (matmul -> bf16, + bias -> bf16), which the reference-generated fixtures pin; every wider linear below rounds once
        h = ops.linear(rows, self._proj_in_padded, None).view(B, lt * lh * lw, self.embed_dim) + self.w["proj_in.bias"]
        if self.with_cls_token:
            h = torch.cat((self.w["cls_token"].expand(B, -1, -1), h), dim=1)
        return h + self._pos_embed((lt, lh, lw))

    def attn_inputs(self, i: int, h: torch.Tensor, batch: int) -> torch.Tensor:
        """`Attention.forward` up to the attention call (:281-292) on token rows `[batch * N, D]` -> q | k | v `[batch * N, 3 D]`."""
        w, p = self.w, f"blocks.{i}."
        y = h if self.ln_in_attn else ops.layernorm(h, LN_EPS, gamma=w[p + "norm1.weight"], beta=w[p + "norm1.bias"])
        qkv = ops.linear(y, w[p + "attn.qkv.weight"], w.get(p + "attn.qkv.bias"))
        if self.ln_in_attn:
            ops.vit_head_prep(qkv, batch=batch, heads=self.num_heads, cls_tokens=self.cls_token_nums, norm=True, eps=LN_EPS)
        return qkv

    def attention(self, qkv: torch.Tensor, batch: int) -> torch.Tensor:
        D = self.embed_dim
        return ops.vit_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], batch=batch, heads=self.num_heads)

    def block_tail(self, i: int, h: torch.Tensor, o: torch.Tensor) -> torch.Tensor:
        """The rest of `Block.forward` (:344-345): h + proj(o), then h + mlp(norm2(h))."""
        w, p = self.w, f"blocks.{i}."
        h = ops.linear(o, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"], epilogue=_hip.IFX_EPI_RESIDUAL, residual=h)
        y = ops.layernorm(h, LN_EPS, gamma=w[p + "norm2.weight"], beta=w[p + "norm2.bias"])
        y = ops.linear(y, w[p + "mlp.fc1.weight"], w[p + "mlp.fc1.bias"], epilogue=_hip.IFX_EPI_GELU_ERF)
        return ops.linear(y, w[p + "mlp.fc2.weight"], w[p + "mlp.fc2.bias"], epilogue=_hip.IFX_EPI_RESIDUAL, residual=h)

    def block(self, i: int, h: torch.Tensor, batch: int) -> torch.Tensor:
        """`Block.forward` on token rows `[batch * N, D]`."""
        return self.block_tail(i, h, self.attention(self.attn_inputs(i, h, batch), batch))

    def head(self, h: torch.Tensor, batch: int, latent: Tuple[int, int, int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """:704-715 on token rows `[batch * N, D]` (the class rows ride along and are skipped by the convolution)."""
        w = self.w
        y = ops.layernorm(h, LN_EPS, gamma=w["norm.weight"], beta=w["norm.bias"])
        if self.use_final_proj:
            y = ops.linear(y, w["final_proj.weight"], w["final_proj.bias"])
            y = ops.layernorm(y, LN_EPS, gamma=w["final_norm.weight"], beta=w["final_norm.bias"])
        return ops.vit_unpatch_conv(y, w["last_layer.weight"], w["last_layer.bias"], batch=batch, cls_tokens=self.cls_token_nums,
                                    latent=latent, patch=(self.patch_length, self.patch_size, self.patch_size), out=out)

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`out`: a contiguous `[B, 3, lT pT, lH pH, lW pW]` bf16 tensor the last kernel writes instead of a fresh one."""
        B, latent = x.shape[0], tuple(x.shape[2:])
        h = self.embed(x).reshape(-1, self.embed_dim)
        for i in range(self.depth):
            h = self.block(i, h, B)
        return self.head(h, B, latent, out)

    __call__ = forward


class HipMagiVAEDecoder:
    """The decode side of `ViTVAE(ddconfig, model_type='vit')` (vae_model.py:222-329): `.decoder` is a HipViTDecoder, `.decode(x)` applies
    the T == 1 rule, the state dict is the reference's with the `decoder.` prefix (`encoder.*` keys are ignored: the encoder is not
    built).  `TileProcessor(decoder=vae.decode, ...)` of the reference can call it as it calls the torch module."""

    def __init__(self, ddconfig: dict, model_type: str = "vit", device="cuda"):
        if model_type != "vit":
            raise NotImplementedError(f"HipMagiVAEDecoder: model_type {model_type!r} (the reference imports 'vit_ncthw' from a package "
                                      "that is not part of it)")
        self.decoder = HipViTDecoder(**ddconfig, device=device)
        self._temporal_downsample_factor = ddconfig.get("patch_length", 1)
        self._spatial_downsample_factor = ddconfig.get("patch_size", 8)
        self.max_rows_per_forward = MAX_ROWS_PER_FORWARD
        self._tile_cache: Dict[tuple, "_ChunkPlan"] = {}

    @property
    def spatial_downsample_factor(self):
        return self._spatial_downsample_factor

    @property
    def temporal_downsample_factor(self):
        return self._temporal_downsample_factor

    def load_state_dict(self, W: Dict[str, torch.Tensor]) -> None:
        self.decoder.load_state_dict(W, prefix="decoder.")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"decoder." + k: v for k, v in self.decoder.state_dict().items()}

    @property
    def allow_spatial_tiling(self):
        return False               # as ViTVAE (vae_model.py:331-333)

    def encode(self, x, sample_posterior=True):
        raise NotImplementedError("HipMagiVAEDecoder: the ViT encoder is not built (decode only)")

    def tiled_encode_3d(self, x, *args, **kwargs):
        raise NotImplementedError("HipMagiVAEDecoder: the ViT encoder is not built (decode only)")

    def decode(self, x: torch.Tensor) -> torch.Tensor:
        """`[N, C, T, H, W]` latents -> pixels; a single latent frame yields a single pixel frame (vae_model.py:300-308)."""
        out = self.decoder(x)
        return out[:, :, :1, :, :] if x.shape[2] == 1 else out

    # ---- chunk decode -----------------------------------------------------------------------------------------------------------------
    def tile_plan(self, latent_shape, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length: int = 16,
                  spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0,
                  allow_spatial_tiling: bool = None) -> _tiles.TilePlan:
        """The tiles `tiled_decode_3d` cuts latents of this shape into (host integers only).  `allow_spatial_tiling=None` falls back to
        the property, and without spatial tiling the spatial tile is 100000 px, as upstream (vae_model.py:208-211)."""
        allow_spatial_tiling = allow_spatial_tiling if allow_spatial_tiling is not None else self.allow_spatial_tiling
        if not allow_spatial_tiling:
            tile_sample_min_height = tile_sample_min_width = 100000
        return _tiles.plan_tiles(latent_shape, tile_sample_min_length, tile_sample_min_height, tile_sample_min_width,
                                 spatial_tile_overlap_factor, temporal_tile_overlap_factor, self._spatial_downsample_factor,
                                 self._temporal_downsample_factor)

    def _chunk_plan(self, shape, tile_sample_min_length, tile_sample_min_height, tile_sample_min_width, spatial_tile_overlap_factor,
                    temporal_tile_overlap_factor, allow_spatial_tiling, max_rows, device) -> "_ChunkPlan":
        key = (tuple(shape), tile_sample_min_length, tile_sample_min_height, tile_sample_min_width, spatial_tile_overlap_factor,
               temporal_tile_overlap_factor, allow_spatial_tiling, max_rows, str(device))
        cp = self._tile_cache.get(key)
        if cp is None:
            N = shape[0]
            plan = self.tile_plan(shape, tile_sample_min_height, tile_sample_min_width, tile_sample_min_length, spatial_tile_overlap_factor,
                                  temporal_tile_overlap_factor, allow_spatial_tiling)
            pT, cls = self._temporal_downsample_factor, self.decoder.cls_token_nums
            # the decoder writes patch_length frames for a single latent frame; `decode` keeps the first: the blend reads it in place
            pitch = tuple((e - b) * pT for b, e in plan.axes[0].spans)
            offsets, runs, at = [0] * len(plan.tiles), [], 0
            for latent, members in plan.groups().items():
                rows = N * (latent[0] * latent[1] * latent[2] + cls)
                per = max(1, max_rows // rows)
                size = N * 3 * latent[0] * pT * latent[1] * self._spatial_downsample_factor * latent[2] * self._spatial_downsample_factor
                for i in range(0, len(members), per):
                    run = members[i:i + per]
                    runs.append((latent, tuple(run), at))
                    for j, m in enumerate(run):
                        offsets[m] = at + j * size
                    at += len(run) * size
            desc = _tiles.plan_blend_table(plan, N, offsets=offsets, frame_pitch=pitch)
            cp = self._tile_cache[key] = _ChunkPlan(plan, desc, desc.tensor(device), torch.empty(desc.arena_elements, dtype=BF16, device=device),
                                                    tuple(runs))
        return cp

    def tiled_decode_3d(self, x: torch.Tensor, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length: int = 16,
                        spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, allow_spatial_tiling: bool = None,
                        verbose: bool = False, parallel_group=None, uint8_output: bool = False,
                        max_rows_per_forward: Optional[int] = None) -> torch.Tensor:
        """`ViTVAE.tiled_decode_3d` (vae_model.py:179-219) with `TileProcessor.tiled_decode` behind it: `[N, C, T, H, W]` latents -> the
        blended chunk `[N, 3, T', H', W']` in bf16, or with `uint8_output` the `[(N T'), 3, H', W']` uint8 frames of `VaeHelper.decode`
        (the bf16 tensor is then never written).  The blends are the reference's eager three-rounding bf16 chain (what
        `torch.compile`d blends round to on a GPU is not pinned).

        Tiles of one latent shape go through the decoder as one batch (tile axis folded with N), split only where a forward would exceed
        `max_rows_per_forward` token rows (default: `self.max_rows_per_forward`; a single tile always runs).  The largest activation of a
        forward is fc1's output, rows x 4 embed_dim x 2 bytes: 512 MiB at the default 65536 rows and the published width, with the
        qkv rows (rows x 3 embed_dim x 2 bytes) alive beside the residual stream.  Plans, descriptor tables and arenas are cached per
        (input shape, arguments); `verbose` is accepted and ignored (no progress bar)."""
        if parallel_group is not None:
            raise NotImplementedError("HipMagiVAEDecoder.tiled_decode_3d: parallel_group (the tile-parallel gather over a process group "
                                      "is not built)")
        if not x.is_cuda:
            raise _hip.HipKernelError(f"HipMagiVAEDecoder: input is on {x.device}; inferix_amd runs on the GPU only")
        allow_spatial_tiling = bool(allow_spatial_tiling if allow_spatial_tiling is not None else self.allow_spatial_tiling)
        max_rows = int(self.max_rows_per_forward if max_rows_per_forward is None else max_rows_per_forward)
        cp = self._chunk_plan(x.shape, tile_sample_min_length, tile_sample_min_height, tile_sample_min_width, spatial_tile_overlap_factor,
                              temporal_tile_overlap_factor, allow_spatial_tiling, max_rows, x.device)
        N, C = x.shape[:2]
        pT, pS = self._temporal_downsample_factor, self._spatial_downsample_factor
        for latent, run, at in cp.runs:
            parts = []
            for m in run:
                (t0, t1), (h0, h1), (w0, w1) = cp.plan.latent_span(cp.plan.tiles[m])
                parts.append(x[:, :, t0:t1, h0:h1, w0:w1])
            z = torch.stack(parts).reshape(len(run) * N, C, *latent)
            shape = (len(run) * N, 3, latent[0] * pT, latent[1] * pS, latent[2] * pS)
            n = shape[0] * shape[1] * shape[2] * shape[3] * shape[4]
            self.decoder(z, out=cp.arena[at:at + n].view(shape))
        out, out_u8 = ops.vit_tile_blend(cp.arena, cp.desc, cp.table, out=not uint8_output, out_u8=bool(uint8_output))
        return out_u8 if uint8_output else out


class _ChunkPlan:
    def __init__(self, plan, desc, table, arena, runs):
        self.plan, self.desc, self.table, self.arena, self.runs = plan, desc, table, arena, runs


class VaeHelper:
    """`VaeHelper` of inferix/pipeline/magi/video_process.py: `decode` only (`get_vae` and `encode` load or run what is not built)."""

    @staticmethod
    def decode(chunk: torch.Tensor, vae: HipMagiVAEDecoder, tile_sample_min_height: int = 256, tile_sample_min_width: int = 256,
               spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, tile_sample_min_length: int = 16,
               allow_spatial_tiling: bool = True, uint8_output: bool = True, parallel_group=None) -> torch.Tensor:
        """:155-200: `[N, C, T, H, W]` latents -> `[(N T'), 3, H', W']` frames, uint8 (`bf16(bf16(x 127.5) + 127.5)`, clamp, truncation,
        evaluated by the blend kernel) or bf16."""
        if not isinstance(vae, HipMagiVAEDecoder):
            raise TypeError(f"VaeHelper.decode: vae is {type(vae).__name__}; the HIP chunk decode is HipMagiVAEDecoder's")
        out = vae.tiled_decode_3d(chunk, tile_sample_min_height=tile_sample_min_height, tile_sample_min_width=tile_sample_min_width,
                                  spatial_tile_overlap_factor=spatial_tile_overlap_factor,
                                  temporal_tile_overlap_factor=temporal_tile_overlap_factor, tile_sample_min_length=tile_sample_min_length,
                                  allow_spatial_tiling=allow_spatial_tiling, parallel_group=parallel_group, uint8_output=uint8_output)
        if uint8_output:
            return out
        N, ch, T, H, W = out.shape
        return out.permute(0, 2, 1, 3, 4).reshape(N * T, ch, H, W)

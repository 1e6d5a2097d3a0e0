"""MAGI-1 ViT-VAE on MI355X: one latent tile -> pixels (BASELINE config 5, PER_BLOCK decode), and pixels -> the clean latents of a
prefix video (image-to-video, video continuation).

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
are not built.  Checkpoint download stays with the caller.

The chunk decode around the tiles (`ViTVAE.tiled_decode_3d` vae_model.py:179-219, `TileProcessor.tiled_decode`
distributed/parallelism/tile_parallel.py:348-448, `VaeHelper.decode` pipeline/magi/video_process.py:155-200) is
`HipMagiVAEDecoder.tiled_decode_3d`: the tiles of a chunk are grouped by latent shape (magi/tiles.py), every group is one batched decoder
forward whose last kernel writes into one arena, and one ifx_vit_tile_blend launch blends, crops, concatenates and converts.

The encode side (`ViTEncoder.forward` vae_module.py:514-558, `ViTVAE.encode` vae_model.py:259-288, `ViTVAE.tiled_encode_3d` :137-177,
`TileProcessor.tiled_encode` tile_parallel.py:254-346, `VaeHelper.encode` video_process.py:113-153, `encode_prefix_video` :279-312):
`HipViTEncoder` shares the blocks with the decoder (`_HipViTBlocks`); its front is ifx_vit_patch_rows + one GEMM whose residual is the
positional table, its tail ifx_vit_latent_head.  `HipMagiVAEDecoder.tiled_encode_3d` groups the tiles by pixel shape, runs one batched
encoder forward per group into an arena of tile latents, and ifx_vit_latent_blend runs the reference's IN-PLACE blend chain on it (a tile
against its already blended neighbours: not the decode's rule); crop and concatenation are slices.
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


class _HipViTBlocks:
    """What `ViTEncoder` and `ViTDecoder` share: the constructor's refusals, the block weights' names and shapes, the positional table and
    `Block.forward` (the same `Block`, `Attention` and `Mlp` classes on both sides of the reference)."""

    def _init_blocks(self, who, video_size, video_length, patch_size, patch_length, z_chans, embed_dim, depth, num_heads, mlp_ratio,
                     qkv_bias, qk_scale, norm_layer, with_cls_token, ln_in_attn, use_rope, device):
        if norm_layer is not None and norm_layer is not torch.nn.LayerNorm:
            raise NotImplementedError(f"{who}: norm_layer other than nn.LayerNorm")
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError(f"{who}: head size {embed_dim / num_heads:g} (ifx_vit_attention is built for 64)")
        if use_rope:
            raise NotImplementedError(f"{who}: use_rope=True raises in the reference's own forward (vae_module.py:289-291 broadcasts "
                                      "the tables against a 5-D slice); there is no result to reproduce")
        if qk_scale is not None:
            raise NotImplementedError(f"{who}: qk_scale (the reference's Attention ignores it too)")
        self._who = who
        self.device = torch.device(device)
        self.embed_dim, self.depth, self.num_heads, self.z_chans = embed_dim, depth, num_heads, z_chans
        self.patch_size, self.patch_length = patch_size, patch_length
        self.latent_size, self.latent_length = video_size // patch_size, video_length // patch_length
        self.hidden = int(embed_dim * mlp_ratio)
        self.qkv_bias, self.ln_in_attn, self.with_cls_token = qkv_bias, ln_in_attn, with_cls_token
        self.cls_token_nums = 1 if with_cls_token else 0
        self.w: Dict[str, torch.Tensor] = {}
        self._pos_embed_host: Optional[torch.Tensor] = None
        self._pos_cache: Dict[Tuple[int, int, int], torch.Tensor] = {}

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def _stem_expected(self) -> Dict[str, Tuple[int, ...]]:
        D = self.embed_dim
        n_pos = self.latent_length * self.latent_size * self.latent_size + self.cls_token_nums
        return {"pos_embed": (1, n_pos, D), "norm.weight": (D,), "norm.bias": (D,)}

    def _block_expected(self) -> Dict[str, Tuple[int, ...]]:
        D, hid = self.embed_dim, self.hidden
        s = {}
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
        return s

    def _load(self, W: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
        w = {}
        for k, shape in self._expected().items():
            if prefix + k not in W:
                raise KeyError(f"{self._who}.load_state_dict: missing {prefix + k}")
            t = W[prefix + k]
            if tuple(t.shape) != shape:
                raise ValueError(f"{self._who}.load_state_dict: {prefix + k} has shape {tuple(t.shape)}, expected {shape}")
            w[k] = t.detach().to(self.device, BF16).contiguous()
        self.w = w
        self._pos_embed_host = w["pos_embed"].cpu()
        self._pos_cache = {}
        return w

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
                    raise NotImplementedError(f"{self._who}: the reference's resize drops row 0 of pos_embed, it needs the class token")
                D = self.embed_dim
                vol = pe[:, 1:, :].reshape(1, *trained, D).permute(0, 4, 1, 2, 3)
                vol = F.interpolate(vol, size=latent, mode="trilinear", align_corners=False)
                pe = torch.cat((pe[:, 0:1, :], vol.permute(0, 2, 3, 4, 1).reshape(1, -1, D)), dim=1)
            pe = self._pos_cache[latent] = pe[0].to(self.device).contiguous()
        return pe

    # ---- Block.forward ----------------------------------------------------------------------------------------------------------------
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


class HipViTDecoder(_HipViTBlocks):
    """`ViTDecoder(**ddconfig)` with `.forward(x: [B, z_chans, lT, lH, lW]) -> [B, 3, lT pT, lH pH, lW pW]` (bf16, on the device) and the
    reference's state-dict keys: `proj_in`, `cls_token`, `pos_embed`, `blocks.N.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}`,
    `norm`, `final_proj`, `final_norm`, `last_layer`."""

    def __init__(self, video_size=256, video_length=16, patch_size=8, patch_length=4, in_chans=3, z_chans=4, double_z=True, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=None, with_cls_token=True, norm_code=False, ln_in_attn=False, conv_last_layer=False,
                 use_rope=False, use_final_proj=False, device="cuda"):
        assert conv_last_layer is True, "Only support conv_last_layer=True"           # as upstream (:643)
        self._init_blocks("HipViTDecoder", video_size, video_length, patch_size, patch_length, z_chans, embed_dim, depth, num_heads, mlp_ratio,
                          qkv_bias, qk_scale, norm_layer, with_cls_token, ln_in_attn, use_rope, device)
        self.use_final_proj = use_final_proj
        patch_volume = patch_size * patch_size * patch_length
        self.unpatch_channels = 4 if use_final_proj else embed_dim // patch_volume
        if self.unpatch_channels != 4 or (not use_final_proj and embed_dim != 4 * patch_volume):
            raise NotImplementedError(f"HipViTDecoder: {embed_dim} / {patch_volume} un-patch channels (ifx_vit_unpatch_conv is built for 4)")
        self._proj_in_padded: Optional[torch.Tensor] = None

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def _expected(self) -> Dict[str, Tuple[int, ...]]:
        D = self.embed_dim
        s = {"proj_in.weight": (D, self.z_chans), "proj_in.bias": (D,), **self._stem_expected(), "last_layer.weight": (3, 4, 3, 3, 3),
             "last_layer.bias": (3,), **self._block_expected()}
        if self.use_final_proj:
            n = 4 * self.patch_size * self.patch_size * self.patch_length
            s["final_proj.weight"], s["final_proj.bias"] = (n, D), (n,)
            s["final_norm.weight"], s["final_norm.bias"] = (n,), (n,)
        return s

    def load_state_dict(self, W: Dict[str, torch.Tensor], prefix: str = "") -> None:
        w = self._load(W, prefix)
        pad = torch.zeros(self.embed_dim, 64, dtype=BF16, device=self.device)        # K = z_chans padded to one 64-wide GEMM K-step
        pad[:, :self.z_chans] = w["proj_in.weight"]
        self._proj_in_padded = pad

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


class HipViTEncoder(_HipViTBlocks):
    """`ViTEncoder(**ddconfig)` (vae_module.py:409-558) with `.forward(x: [B, 3, T, H, W]) -> [B, C2, lT, lH, lW]` moments (bf16, on the
    device; C2 = 2 z_chans, z_chans without `double_z`) and the reference's state-dict keys: `patch_embed.proj`, `cls_token`, `pos_embed`,
    `blocks.N.*`, `norm`, `last_layer`.  x is bf16 in [-1, 1], any other float type (cast), or uint8 pixels, which the patch kernel
    normalises as `VaeHelper.encode` does; any strided view is read in place.

    The patch embedding is one GEMM over the rows of ifx_vit_patch_rows with the positional table as its residual:
    bf16(bf16(fp32 acc + bias) + pos), the two roundings of the reference's bf16 Conv3d and `x + pos_embed`."""

    def __init__(self, video_size=256, video_length=16, patch_size=8, patch_length=4, in_chans=3, z_chans=4, double_z=True, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer=None, with_cls_token=True, norm_code=False, ln_in_attn=False, conv_last_layer=False,
                 use_rope=False, use_final_proj=False, device="cuda"):
        # conv_last_layer and use_final_proj are the decoder's; upstream overwrites the first and never reads the second (:440)
        if in_chans != 3:
            raise NotImplementedError(f"HipViTEncoder: in_chans {in_chans} (ifx_vit_patch_rows is built for 3)")
        self._init_blocks("HipViTEncoder", video_size, video_length, patch_size, patch_length, z_chans, embed_dim, depth, num_heads, mlp_ratio,
                          qkv_bias, qk_scale, norm_layer, with_cls_token, ln_in_attn, use_rope, device)
        self.norm_code = bool(norm_code)
        self.out_channels = z_chans * 2 if double_z else z_chans
        self.latent_channels = self.out_channels // 2          # `DiagonalGaussianDistribution` halves the moments whatever double_z says
        self.patch = (patch_length, patch_size, patch_size)
        self.patch_k = 3 * patch_length * patch_size * patch_size
        self._proj_flat: Optional[torch.Tensor] = None
        self._pos_rows: Dict[Tuple[Tuple[int, int, int], int], torch.Tensor] = {}

    def _expected(self) -> Dict[str, Tuple[int, ...]]:
        D = self.embed_dim
        return {"patch_embed.proj.weight": (D, 3) + self.patch, "patch_embed.proj.bias": (D,), **self._stem_expected(),
                "last_layer.weight": (self.out_channels, D), "last_layer.bias": (self.out_channels,), **self._block_expected()}

    def load_state_dict(self, W: Dict[str, torch.Tensor], prefix: str = "") -> None:
        w = self._load(W, prefix)
        self._proj_flat = w["patch_embed.proj.weight"].flatten(1).contiguous()
        self._pos_rows = {}

    # ---- forward ------------------------------------------------------------------------------------------------------------------------
    def latent_shape(self, pixels: Tuple[int, int, int]) -> Tuple[int, int, int]:
        """floor(extent / patch) per axis, what the strided convolution gives."""
        return tuple(int(e) // p for e, p in zip(pixels, self.patch))

    def _video(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise _hip.HipKernelError(f"HipViTEncoder: input is on {x.device}; inferix_amd runs on the GPU only")
        if not self.w:
            raise RuntimeError("HipViTEncoder: no weights loaded")
        assert x.dim() == 5 and x.shape[1] == 3, x.shape
        return x if x.dtype in (BF16, torch.uint8) else x.to(BF16)

    def patch_rows(self, x: torch.Tensor, tiles=None) -> Tuple[torch.Tensor, int, Tuple[int, int, int]]:
        """(rows `[batch * (cls + tokens), K]`, batch, latent) for the whole video or for `tiles` = [(t0, h0, w0, Te, He, We)] of one
        latent shape (batch = tiles x N, tile-major)."""
        x = self._video(x)
        if tiles is None:
            tiles = [(0, 0, 0) + tuple(x.shape[2:])]
        latent = self.latent_shape(tiles[0][3:])
        rows = ops.vit_patch_rows(x, tiles, latent, self.patch, cls_tokens=self.cls_token_nums)
        return rows, len(tiles) * x.shape[0], latent

    def embed_rows(self, rows: torch.Tensor, batch: int, latent: Tuple[int, int, int]) -> torch.Tensor:
        """:517-536 on patch rows -> token rows `[batch * (cls + tokens), D]`."""
        key = (latent, batch)
        pos = self._pos_rows.get(key)
        if pos is None:
            self._pos_rows.clear()              # one shape at a time: a batched forward's table is as large as its token rows
            pos = self._pos_rows[key] = self._pos_embed(latent).repeat(batch, 1)
        h = ops.linear(rows, self._proj_flat, self.w["patch_embed.proj.bias"], epilogue=_hip.IFX_EPI_RESIDUAL, residual=pos)
        if self.with_cls_token:
            h.view(batch, -1, self.embed_dim)[:, 0] = self.w["cls_token"][0, 0] + self._pos_embed(latent)[0]
        return h

    def embed(self, x: torch.Tensor, tiles=None) -> torch.Tensor:
        """-> token rows `[B, cls + tokens, D]`."""
        rows, batch, latent = self.patch_rows(x, tiles)
        return self.embed_rows(rows, batch, latent).view(batch, -1, self.embed_dim)

    def head(self, h: torch.Tensor, batch: int, latent: Tuple[int, int, int], out: Optional[torch.Tensor] = None,
             store_channels: Optional[int] = None) -> torch.Tensor:
        """:542-557 on token rows `[batch * N, D]` -> `[batch, store_channels, lT, lH, lW]` (default: every moment channel)."""
        w = self.w
        return ops.vit_latent_head(h, w["norm.weight"], w["norm.bias"], w["last_layer.weight"], w["last_layer.bias"], batch=batch,
                                   cls_tokens=self.cls_token_nums, latent=latent, norm_code=self.norm_code, eps=LN_EPS,
                                   store_channels=store_channels, out=out)

    def forward(self, x: torch.Tensor, tiles=None, out: Optional[torch.Tensor] = None, store_channels: Optional[int] = None) -> torch.Tensor:
        rows, batch, latent = self.patch_rows(x, tiles)
        h = self.embed_rows(rows, batch, latent)
        for i in range(self.depth):
            h = self.block(i, h, batch)
        return self.head(h, batch, latent, out, store_channels)

    __call__ = forward


class HipMagiVAEDecoder:
    """`ViTVAE(ddconfig, model_type='vit')` (vae_model.py:222-329): `.decoder` is a HipViTDecoder, `.decode(x)` applies the T == 1 rule, the
    state dict is the reference's with the `decoder.` prefix.  `.encoder` is None until a state dict with encoder weights is loaded
    (`encoder.patch_embed.proj.weight` present; other `encoder.*` keys without it are ignored), then a HipViTEncoder behind `.encode` and
    `.tiled_encode_3d`.  `TileProcessor(decoder=vae.decode, ...)` of the reference can call it as it calls the torch module.  The class
    keeps its name from the time it decoded only."""

    def __init__(self, ddconfig: dict, model_type: str = "vit", device="cuda"):
        if model_type != "vit":
            raise NotImplementedError(f"HipMagiVAEDecoder: model_type {model_type!r} (the reference imports 'vit_ncthw' from a package "
                                      "that is not part of it)")
        self.decoder = HipViTDecoder(**ddconfig, device=device)
        self.encoder: Optional[HipViTEncoder] = None
        self._ddconfig, self._device = dict(ddconfig), device
        self._encode_cache: Dict[tuple, "_EncodePlan"] = {}
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
        if "encoder.patch_embed.proj.weight" in W:
            enc = HipViTEncoder(**self._ddconfig, device=self._device)
            enc.load_state_dict(W, prefix="encoder.")
            self.encoder = enc
            self._encode_cache = {}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {"decoder." + k: v for k, v in self.decoder.state_dict().items()}
        if self.encoder is not None:
            sd.update({"encoder." + k: v for k, v in self.encoder.state_dict().items()})
        return sd

    def load_synthetic(self, seed: int = 0, encoder: bool = True) -> None:
        """Random weights on both sides (benchmarks): the decoder's from `seed`, the encoder's from `seed + 1`."""
        self.decoder.load_synthetic(seed)
        if encoder:
            self.encoder = HipViTEncoder(**self._ddconfig, device=self._device)
            self.encoder.load_synthetic(seed + 1)
            self._encode_cache = {}

    @property
    def allow_spatial_tiling(self):
        return False               # as ViTVAE (vae_model.py:331-333)

    def _need_encoder(self, what: str) -> HipViTEncoder:
        if self.encoder is None:
            raise NotImplementedError(f"HipMagiVAEDecoder.{what}: no encoder weights are loaded (load_state_dict builds the ViT encoder "
                                      "when the state dict holds encoder.patch_embed.proj.weight)")
        return self.encoder

    @staticmethod
    def _sample(moments: torch.Tensor, generator=None) -> torch.Tensor:
        """`DiagonalGaussianDistribution(moments).sample()` (vae_module.py:722-735) with the noise drawn on the device."""
        mean, logvar = torch.chunk(moments, 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return mean + std * torch.randn(mean.shape, dtype=mean.dtype, device=mean.device, generator=generator)

    def encode(self, x, sample_posterior=True, generator=None):
        """`ViTVAE.encode` (vae_model.py:259-288): `[N, 3, T, H, W]` -> `[N, z_chans, lT, lH, lW]`, the posterior's sample or (with
        `sample_posterior=False`) its mode; a single frame is expanded to 4 by stride and yields a single latent frame."""
        enc = self._need_encoder("encode")
        single = x.shape[2] == 1 and self._temporal_downsample_factor > 1
        moments = enc(x.expand(-1, -1, 4, -1, -1) if single else x)
        z = self._sample(moments, generator) if sample_posterior else torch.chunk(moments, 2, dim=1)[0]
        return (z[:, :, :1] if single else z).to(moments.dtype)

    # ---- prefix-video encode ----------------------------------------------------------------------------------------------------------
    def encode_tile_plan(self, video_shape, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length: int = 16,
                         spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0,
                         allow_spatial_tiling: bool = None) -> _tiles.TilePlan:
        """The tiles `tiled_encode_3d` cuts a video of this shape into (host integers only; spans in pixels, extents in latents)."""
        allow_spatial_tiling = allow_spatial_tiling if allow_spatial_tiling is not None else self.allow_spatial_tiling
        if not allow_spatial_tiling:
            tile_sample_min_height = tile_sample_min_width = 100000
        return _tiles.plan_encode_tiles(video_shape, tile_sample_min_length, tile_sample_min_height, tile_sample_min_width,
                                        spatial_tile_overlap_factor, temporal_tile_overlap_factor, self._spatial_downsample_factor,
                                        self._temporal_downsample_factor)

    def _encode_plan(self, shape, args, max_rows, device) -> "_EncodePlan":
        key = (tuple(shape), args, max_rows, str(device))
        ep = self._encode_cache.get(key)
        if ep is None:
            N = shape[0]
            enc = self.encoder
            plan = self.encode_tile_plan(shape, *args)
            z, cls = enc.latent_channels, enc.cls_token_nums
            offsets, runs, at = [0] * len(plan.tiles), [], 0
            for pixels, members in plan.groups().items():
                latent = plan.decoded_shape(plan.tiles[members[0]])
                tokens = latent[0] * latent[1] * latent[2]
                per = max(1, max_rows // (N * (tokens + cls)))
                size = N * z * tokens
                for i in range(0, len(members), per):
                    run = members[i:i + per]
                    runs.append((pixels, latent, tuple(run), at))
                    for j, m in enumerate(run):
                        offsets[m] = at + j * size
                    at += len(run) * size
            desc = _tiles.plan_latent_blend_table(plan, N * z, offsets=offsets)
            ep = self._encode_cache[key] = _EncodePlan(plan, desc, desc.tensor(device), tuple(runs))
        return ep

    def tiled_encode_3d(self, x: torch.Tensor, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length: int = 16,
                        spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, allow_spatial_tiling: bool = None,
                        verbose: bool = False, parallel_group=None, deterministic: bool = True, generator=None,
                        max_rows_per_forward: Optional[int] = None) -> torch.Tensor:
        """`ViTVAE.tiled_encode_3d` (vae_model.py:137-177) with `TileProcessor.tiled_encode` behind it: a video `[N, 3, T, H, W]` (bf16 in
        [-1, 1], or uint8 pixels) -> the blended latents `[N, z_chans, T', H', W']` in bf16.

        `deterministic=True` (the default, a deviation from the signature's spirit but not from its use): every tile is encoded to the
        posterior's MODE.  The reference's only caller reaches this method through `VaeHelper.get_vae`, which replaces `encode` by the
        mode-only `patch_vae_encode` (video_process.py:66, 77-110).  With `deterministic=False` every tile is a sample, as the unpatched
        `ViTVAE.encode` gives.

        Tiles of one pixel shape go through the encoder as one batch (tile axis folded with N), split only where a forward would exceed
        `max_rows_per_forward` token rows.  The last kernel of a forward writes the tile latents into one arena, ifx_vit_latent_blend
        runs the reference's in-place blend chain on it, crop and concatenation are slices of the arena.  `verbose` is accepted and
        ignored."""
        enc = self._need_encoder("tiled_encode_3d")
        if parallel_group is not None:
            raise NotImplementedError("HipMagiVAEDecoder.tiled_encode_3d: parallel_group (the tile-parallel gather over a process group "
                                      "is not built)")
        if not x.is_cuda:
            raise _hip.HipKernelError(f"HipMagiVAEDecoder: input is on {x.device}; inferix_amd runs on the GPU only")
        allow_spatial_tiling = bool(allow_spatial_tiling if allow_spatial_tiling is not None else self.allow_spatial_tiling)
        max_rows = int(self.max_rows_per_forward if max_rows_per_forward is None else max_rows_per_forward)
        args = (tile_sample_min_height, tile_sample_min_width, tile_sample_min_length, spatial_tile_overlap_factor,
                temporal_tile_overlap_factor, allow_spatial_tiling)
        ep = self._encode_plan(x.shape, args, max_rows, x.device)
        plan, N, z, pT = ep.plan, x.shape[0], enc.latent_channels, self._temporal_downsample_factor
        arena = torch.empty(ep.desc.arena_elements, dtype=BF16, device=x.device)
        for pixels, latent, run, at in ep.runs:
            video, tiles = x, []
            for m in run:
                (t0, _), (h0, _), (w0, _) = plan.latent_span(plan.tiles[m])
                tiles.append((t0, h0, w0) + tuple(pixels))
            if pixels[0] == 1 and pT > 1:
                # `ViTVAE.encode`'s T == 1 rule: the frame four times, by stride; only the last temporal index can hold a single frame
                if 4 // pT != 1:
                    raise NotImplementedError(f"HipMagiVAEDecoder.tiled_encode_3d: a single-frame tile with patch_length {pT}")
                t0 = tiles[0][0]
                assert all(t[0] == t0 for t in tiles)
                video = x[:, :, t0:t0 + 1].expand(-1, -1, 4, -1, -1)
                tiles = [(0, h0, w0, 4, He, We) for _, h0, w0, _, He, We in tiles]
            B = len(run) * N
            slot = arena[at:at + B * z * latent[0] * latent[1] * latent[2]].view(B, z, *latent)
            if deterministic:
                enc(video, tiles, out=slot, store_channels=z)
            else:
                slot.copy_(self._sample(enc(video, tiles), generator))
        ops.vit_latent_blend(arena, ep.desc, ep.table)
        return assemble_encoded_tiles(arena, plan, ep.desc.offsets, N, z)

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
                        verbose: bool = False, parallel_group=None, uint8_output=False,
                        max_rows_per_forward: Optional[int] = None) -> torch.Tensor:
        """`ViTVAE.tiled_decode_3d` (vae_model.py:179-219) with `TileProcessor.tiled_decode` behind it: `[N, C, T, H, W]` latents -> the
        blended chunk `[N, 3, T', H', W']` in bf16, or with `uint8_output` the `[(N T'), 3, H', W']` uint8 frames of `VaeHelper.decode`
        (the bf16 tensor is then never written).  `uint8_output="hwc"`: the same uint8 values channel-last, `[N, T', H', W', 3]`, what a
        frame consumer takes, written by the blend itself; a uint8 TENSOR of that shape in place of "hwc" is filled in place and
        returned (a stream's slot buffer).  The blends are the reference's eager three-rounding bf16 chain (what `torch.compile`d blends
        round to on a GPU is not pinned).

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
        hwc_out = uint8_output if isinstance(uint8_output, torch.Tensor) else None
        hwc = hwc_out is not None or isinstance(uint8_output, str)
        if isinstance(uint8_output, str) and uint8_output != "hwc":
            raise ValueError(f"HipMagiVAEDecoder.tiled_decode_3d: uint8_output is True, False, 'hwc' or a uint8 tensor to fill, "
                             f"got {uint8_output!r}")
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
        if hwc:
            return ops.vit_tile_blend(cp.arena, cp.desc, cp.table, out=False, out_hwc=True if hwc_out is None else hwc_out)[2]
        out, out_u8 = ops.vit_tile_blend(cp.arena, cp.desc, cp.table, out=not uint8_output, out_u8=bool(uint8_output))
        return out_u8 if uint8_output else out


def assemble_encoded_tiles(arena: torch.Tensor, plan: _tiles.TilePlan, offsets, batch: int, channels: int) -> torch.Tensor:
    """The tail of `tiled_encode` (tile_parallel.py:329-346) on the blended arena: every tile `[batch, channels, T_k, H_k, W_k]` at its
    offset cropped to the limits, the crops concatenated along w, h and t."""
    lim = tuple(a.limit for a in plan.axes)
    nt, nh, nw = plan.grid
    frames = []
    for f in range(nt):
        rows = []
        for i in range(nh):
            row = []
            for j in range(nw):
                k = (f * nh + i) * nw + j
                T_, H_, W_ = plan.decoded_shape(plan.tiles[k])
                tile = arena[offsets[k]:offsets[k] + batch * channels * T_ * H_ * W_].view(batch, channels, T_, H_, W_)
                row.append(tile[:, :, :lim[0], :lim[1], :lim[2]])
            rows.append(torch.cat(row, dim=4))
        frames.append(torch.cat(rows, dim=3))
    return torch.cat(frames, dim=2)


class _ChunkPlan:
    def __init__(self, plan, desc, table, arena, runs):
        self.plan, self.desc, self.table, self.arena, self.runs = plan, desc, table, arena, runs


class _EncodePlan:
    def __init__(self, plan, desc, table, runs):
        self.plan, self.desc, self.table, self.runs = plan, desc, table, runs


class VaeHelper:
    """`VaeHelper` of inferix/pipeline/magi/video_process.py: `encode` and `decode` (`get_vae` loads a checkpoint, which stays with the
    caller)."""

    @staticmethod
    def encode(video: torch.Tensor, vae: "HipMagiVAEDecoder", tile_sample_min_length: int = 16, tile_sample_min_height: int = 256,
               tile_sample_min_width: int = 256, spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0,
               allow_spatial_tiling: bool = True, parallel_group=None) -> torch.Tensor:
        """:113-153: pixels `[N, C, T, H, W]` in [0, 255], uint8 or float, -> latents `[N, z_chans, T', H', W']` in bf16, every tile the
        posterior's mode (the reference's `get_vae` patches `encode` to that).  uint8 pixels are normalised by the patch kernel,
        `bf16(fp32(v) / 127.5 - 1)`; a float video is normalised here by the reference's two operators."""
        if not isinstance(vae, HipMagiVAEDecoder):
            raise TypeError(f"VaeHelper.encode: vae is {type(vae).__name__}; the HIP prefix encode is HipMagiVAEDecoder's")
        assert video.dim() == 5, f"Expected input tensor to have shape (N, C, T, H, W), but got {video.shape}."
        video = video.to(vae.decoder.device)
        if video.dtype != torch.uint8:
            video = ((video / 127.5) - 1.0).bfloat16()
        return vae.tiled_encode_3d(video, tile_sample_min_length=tile_sample_min_length, tile_sample_min_height=tile_sample_min_height,
                                   tile_sample_min_width=tile_sample_min_width, spatial_tile_overlap_factor=spatial_tile_overlap_factor,
                                   temporal_tile_overlap_factor=temporal_tile_overlap_factor, allow_spatial_tiling=allow_spatial_tiling,
                                   parallel_group=parallel_group)

    @staticmethod
    def decode(chunk: torch.Tensor, vae: HipMagiVAEDecoder, tile_sample_min_height: int = 256, tile_sample_min_width: int = 256,
               spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, tile_sample_min_length: int = 16,
               allow_spatial_tiling: bool = True, uint8_output=True, parallel_group=None) -> torch.Tensor:
        """:155-200: `[N, C, T, H, W]` latents -> `[(N T'), 3, H', W']` frames, uint8 (`bf16(bf16(x 127.5) + 127.5)`, clamp, truncation,
        evaluated by the blend kernel) or bf16.  `uint8_output="hwc"` (not upstream): the uint8 frames channel-last, `[N, T', H', W', 3]`;
        a uint8 tensor of that shape in its place is filled and returned."""
        if not isinstance(vae, HipMagiVAEDecoder):
            raise TypeError(f"VaeHelper.decode: vae is {type(vae).__name__}; the HIP chunk decode is HipMagiVAEDecoder's")
        out = vae.tiled_decode_3d(chunk, tile_sample_min_height=tile_sample_min_height, tile_sample_min_width=tile_sample_min_width,
                                  spatial_tile_overlap_factor=spatial_tile_overlap_factor,
                                  temporal_tile_overlap_factor=temporal_tile_overlap_factor, tile_sample_min_length=tile_sample_min_length,
                                  allow_spatial_tiling=allow_spatial_tiling, parallel_group=parallel_group, uint8_output=uint8_output)
        if isinstance(uint8_output, (str, torch.Tensor)) or uint8_output:
            return out
        N, ch, T, H, W = out.shape
        return out.permute(0, 2, 1, 3, 4).reshape(N * T, ch, H, W)


def encode_prefix_video(prefix_video: Optional[torch.Tensor], fps: int, vae: HipMagiVAEDecoder, scale_factor: float,
                        parallel_group=None) -> Optional[torch.Tensor]:
    """`encode_prefix_video` of inferix/pipeline/magi/video_process.py:279-312 with the vae OBJECT in place of a checkpoint path (loading
    stays with the caller, as for decode): frames `[T, H, W, C]` -> the clean latents `[1, z_chans, T', H', W']` x `scale_factor` in
    bf16 that `ChunkSchedule.run(prefix_video=...)` takes.  Tiles of `fps // 2` frames and 256 x 256 pixels at overlap 0.25."""
    if prefix_video is None:
        return None
    video = prefix_video.permute(3, 0, 1, 2).unsqueeze(0)          # THWC -> NCTHW, a view: the patch kernel reads it by stride
    latents = VaeHelper.encode(video, vae, tile_sample_min_height=256, tile_sample_min_width=256, spatial_tile_overlap_factor=0.25,
                               temporal_tile_overlap_factor=0, tile_sample_min_length=fps // 2, allow_spatial_tiling=True,
                               parallel_group=parallel_group)
    return latents * scale_factor


def decode_chunk(chunk: torch.Tensor, vae: HipMagiVAEDecoder, scale_factor: float, tile_sample_min_length: int,
                 parallel_group=None, uint8_output=True) -> torch.Tensor:
    """`decode_chunk` of inferix/pipeline/magi/video_process.py:348-374 with the vae OBJECT in place of a checkpoint path: latents
    `[1, z_chans, T, H, W]` of one finished chunk -> uint8 frames `[T', 3, H', W']`.  Tiles of 256 x 256 pixels at overlap 0.25.
    `uint8_output="hwc"` (not upstream): `[1, T', H', W', 3]`; a uint8 tensor of that shape in its place is filled and returned."""
    form = {} if uint8_output is True else dict(uint8_output=uint8_output)
    return VaeHelper.decode(chunk / scale_factor, vae, tile_sample_min_height=256, tile_sample_min_width=256,
                            spatial_tile_overlap_factor=0.25, temporal_tile_overlap_factor=0,
                            tile_sample_min_length=tile_sample_min_length, allow_spatial_tiling=True, parallel_group=parallel_group, **form)


def post_chunk_process(chunk: torch.Tensor, config, vae: HipMagiVAEDecoder, parallel_group=None) -> torch.Tensor:
    """`post_chunk_process` (:377-388): the decode of a chunk `generate_per_chunk` hands out, temporal tiles of `fps // 2` frames
    (`tile_sample_min_length`).  Upstream's `gc.collect()` / `empty_cache()` behind it is allocator hygiene for small cards and is not mirrored."""
    rc = config.runtime_config
    return decode_chunk(chunk, vae, rc.scale_factor, rc.fps // 2, parallel_group=parallel_group)

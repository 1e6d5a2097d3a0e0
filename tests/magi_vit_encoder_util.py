"""Shared by the MAGI ViT-VAE encoder tests and tools/gen_golden_magi_vit_encoder.py: the encoder configs of the fixtures, the seeded weight
generator (fixtures hold seeds, inputs and outputs, never weights) and plain-torch restatements of
  * `ViTEncoder.forward` (inferix/models/magi/vae/vae_module.py:409-558): the patch convolution through `F.conv3d`, the class token, the
    positional table, the blocks (`magi_vit_util.block_forward`: the same `Block` as the decoder's), the final norm, `last_layer`, the
    channel-first moments and `norm_code`;
  * `ViTVAE.encode` with the posterior's mode (vae_model.py:259-288, the form `VaeHelper.get_vae` patches in);
  * `TileProcessor.tiled_encode` (inferix/distributed/parallelism/tile_parallel.py:254-346): tiles cut in pixels, every tile blended IN
    PLACE against its already blended neighbours, cropped to the limits in latents, concatenated.
On bf16 tensors they evaluate the reference's op chain on the CPU, so they equal the reference-generated fixtures
tests/golden/magi_vitenc_*.npz and magi_enc_tiles_*.npz bit for bit (tests/test_magi_vit_encoder_oracle.py); with dtype float32 the
encoder is the exact-arithmetic evaluation the measured-noise rule takes its floor from.  Nothing here imports oracle/, the reference or
inferix_amd."""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

import magi_vit_util as U
from magi_tiles_util import blend
from magi_vit_util import BF, GOLDEN_DIR, LN_EPS, block_forward, load_fixture, resized_pos_embed, save_fixture  # noqa: F401


@dataclasses.dataclass(frozen=True)
class EncConfig(U.VitConfig):
    """The constructor arguments of `ViTEncoder` that reach the forward (the decoder's plus the two that shape the moments)."""
    norm_code: bool = False
    double_z: bool = True

    @property
    def patch(self) -> Tuple[int, int, int]:
        return (self.patch_length, self.patch_size, self.patch_size)

    @property
    def out_channels(self) -> int:
        return 2 * self.z_chans if self.double_z else self.z_chans


TINY = EncConfig(video_size=32, video_length=8, embed_dim=256, depth=2, num_heads=4, ln_in_attn=True, qkv_bias=True, z_chans=4,
                 use_final_proj=True)
# name -> (config, weight seed, [(input seed, input shape [N, 3, T, H, W])], stages stored for the first input)
CASES = {
    # (a) the trained shape: 2 x 4 x 4 latents + class token = 33 tokens
    "magi_vitenc_a": (TINY, 5100, [(31, (1, 3, 8, 32, 32))], True),
    # (b) the same weights on a resized positional table, latent (1, 5, 3); second input: 10 x 36 x 44 floors to (2, 4, 5)
    "magi_vitenc_b": (TINY, 5100, [(32, (1, 3, 4, 40, 24)), (33, (1, 3, 10, 36, 44))], True),
    # (c) norm1 path at width 1024, 32 moment channels, norm_code
    "magi_vitenc_c": (EncConfig(video_size=32, video_length=8, embed_dim=1024, depth=1, num_heads=16, z_chans=16, norm_code=True), 5200,
                      [(34, (1, 3, 8, 32, 32))], False),
    # (d) one block at the published width and flags: 4 x 8 x 8 latents + class token = 257 tokens
    "magi_vitenc_d": (EncConfig(video_size=64, video_length=16, embed_dim=1024, depth=1, num_heads=16, ln_in_attn=True, qkv_bias=True,
                                z_chans=16, use_final_proj=True), 5300, [(35, (1, 3, 16, 64, 64))], False),
}
FP32_CASES = ("magi_vitenc_a", "magi_vitenc_d")

# name -> (video shape, (tile length, height, width) in pixels, spatial overlap, temporal overlap, video seed, grid, output shape);
# all on the case (a) encoder
TILE_WEIGHT_SEED = 5100
TILE_CASES = {
    # grid 2 x 3 x 2, eight distinct tile shapes, one-latent-wide edge tiles
    "magi_enc_tiles_a": ((1, 3, 12, 56, 40), (8, 32, 32), 0.25, 0.0, 41, (2, 3, 2), (3, 7, 5)),
    # the same video with a temporal blend: grid 3 x 3 x 2
    "magi_enc_tiles_b": ((1, 3, 12, 56, 40), (8, 32, 32), 0.25, 0.5, 41, (3, 3, 2), (3, 7, 5)),
    # the image case: T == 1 in every tile
    "magi_enc_tiles_c": ((1, 3, 1, 56, 40), (8, 32, 32), 0.25, 0.0, 42, (1, 3, 2), (1, 7, 5)),
}


def make_encoder_weights(cfg: EncConfig, seed: int, dtype=BF) -> Dict[str, torch.Tensor]:
    """State dict of `ViTEncoder(**cfg.ctor_kwargs())` under the reference's key names, from one seed; values are bf16-representable."""
    g = torch.Generator().manual_seed(seed)
    D, hid = cfg.embed_dim, int(cfg.embed_dim * cfg.mlp_ratio)
    W: Dict[str, torch.Tensor] = {}

    def rnd(*shape, std=1.0, mean=0.0):
        return (torch.randn(*shape, generator=g) * std + mean).to(BF).to(dtype)

    def linear(name, n_out, n_in, bias=True):
        W[name + ".weight"] = rnd(n_out, n_in, std=n_in ** -0.5)
        if bias:
            W[name + ".bias"] = rnd(n_out, std=0.05)

    def norm(name, n):
        W[name + ".weight"] = rnd(n, std=0.1, mean=1.0)
        W[name + ".bias"] = rnd(n, std=0.05)

    K = 3 * cfg.patch_volume
    W["patch_embed.proj.weight"] = rnd(D, 3, *cfg.patch, std=K ** -0.5)
    W["patch_embed.proj.bias"] = rnd(D, std=0.05)
    if cfg.with_cls_token:
        W["cls_token"] = rnd(1, 1, D, std=0.5)
    lt, lh, lw = cfg.latent
    W["pos_embed"] = rnd(1, lt * lh * lw + cfg.cls, D, std=0.5)
    for i in range(cfg.depth):
        p = f"blocks.{i}."
        if not cfg.ln_in_attn:
            norm(p + "norm1", D)
        linear(p + "attn.qkv", 3 * D, D, bias=cfg.qkv_bias)
        linear(p + "attn.proj", D, D)
        norm(p + "norm2", D)
        linear(p + "mlp.fc1", hid, D)
        linear(p + "mlp.fc2", D, hid)
    norm("norm", D)
    linear("last_layer", cfg.out_channels, D)
    return W


def make_video(seed: int, shape, dtype=BF) -> torch.Tensor:
    """A bf16-representable video in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.5).clamp(-1, 1).to(BF).to(dtype)


def make_pixels(seed: int, shape) -> torch.Tensor:
    """A uint8 video."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, tuple(shape), generator=g, dtype=torch.uint8)


def normalise_pixels(video: torch.Tensor) -> torch.Tensor:
    """`VaeHelper.encode` (inferix/pipeline/magi/video_process.py:140-141) as its three torch operators."""
    video = (video / 127.5) - 1.0
    return video.bfloat16()


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------
def gather_patch_rows(x: torch.Tensor, patch: Tuple[int, int, int]) -> torch.Tensor:
    """`[B, 3, T, H, W]` -> `[B, lT lH lW, 3 pT pH pW]`: the pixels of every patch in the K order (c, t, h, w) of `weight.flatten(1)`;
    trailing pixels that fill no patch are dropped, as a strided convolution drops them."""
    B, C, T, H, W = x.shape
    pt, ph, pw = patch
    lt, lh, lw = T // pt, H // ph, W // pw
    v = x[:, :, :lt * pt, :lh * ph, :lw * pw].reshape(B, C, lt, pt, lh, ph, lw, pw)
    return v.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, lt * lh * lw, C * pt * ph * pw)


def latent_head(W, cfg: EncConfig, h: torch.Tensor, latent: Tuple[int, int, int], taps: Optional[dict] = None) -> torch.Tensor:
    """:542-557 on token rows `[B, cls + tokens, D]` -> moments `[B, C2, lT, lH, lW]`."""
    B = h.shape[0]
    h = F.layer_norm(h, (cfg.embed_dim,), W["norm.weight"], W["norm.bias"], LN_EPS)
    if taps is not None:
        taps["normed"] = h
    h = F.linear(h, W["last_layer.weight"], W["last_layer.bias"])
    if cfg.with_cls_token:
        h = h[:, 1:]
    h = h.reshape(B, *latent, cfg.out_channels).permute(0, 4, 1, 2, 3)
    if cfg.norm_code:
        prev = h.dtype
        h = h.float()
        h = (h / torch.norm(h, dim=1, keepdim=True)).to(prev)
    return h


def encoder_forward(W, cfg: EncConfig, x: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
    """`ViTEncoder.forward`: x `[B, 3, T, H, W]` -> moments `[B, C2, lT, lH, lW]`; `taps` collects the gathered patch rows, the token rows
    after the embedding (`embed`) and after every block (`block{i}`), the head-prep and attention outputs and the normed rows."""
    B = x.shape[0]
    h = F.conv3d(x, W["patch_embed.proj.weight"], W["patch_embed.proj.bias"], stride=cfg.patch)
    latent = tuple(h.shape[2:])
    h = h.flatten(2).transpose(1, 2)
    if cfg.with_cls_token:
        h = torch.cat((W["cls_token"].expand(B, -1, -1), h), dim=1)
    h = h + resized_pos_embed(W["pos_embed"], cfg, latent)
    if taps is not None:
        taps["patch_rows"] = gather_patch_rows(x, cfg.patch)
        taps["embed"] = h
    for i in range(cfg.depth):
        h = block_forward(W, cfg, i, h, latent, taps)
        if taps is not None:
            taps[f"block{i}"] = h
    return latent_head(W, cfg, h, latent, taps).contiguous()


def encode_mode(W, cfg: EncConfig) -> Callable[[torch.Tensor], torch.Tensor]:
    """`ViTVAE.encode(x, sample_posterior=False)` over the restated encoder: one frame is expanded to 4 and gives one latent frame."""
    def encode(x: torch.Tensor) -> torch.Tensor:
        single = x.shape[2] == 1 and cfg.patch_length > 1
        m = encoder_forward(W, cfg, x.expand(-1, -1, 4, -1, -1) if single else x)
        z = torch.chunk(m, 2, dim=1)[0]
        return z[:, :, :1] if single else z
    return encode


# ---- the tile pass --------------------------------------------------------------------------------------------------------------------
class EncodeAxis:
    """One axis of `tiled_encode` (:255-269): tile and stride in PIXELS, blend extent and kept limit in LATENTS, tile count."""

    def __init__(self, size: int, tile_px: int, overlap: float, ds: int):
        self.tile = tile_px
        self.stride = int(tile_px * (1 - overlap))
        tl = tile_px // ds
        self.extent = int(tl * overlap)
        self.limit = tl - self.extent
        self.count = -(-size // self.stride)

    def span(self, k: int) -> slice:
        return slice(k * self.stride, k * self.stride + self.tile)


def encode_axes(shape, tile_px, spatial_overlap: float, temporal_overlap: float, ds=(4, 8, 8)) -> List[EncodeAxis]:
    return [EncodeAxis(shape[-3 + i], tile_px[i], (temporal_overlap, spatial_overlap, spatial_overlap)[i], ds[i]) for i in range(3)]


def encode_tiles(encode, x: torch.Tensor, axes: List[EncodeAxis]) -> dict:
    """Raw tile latents keyed by (f, i, j), encoded in the reference's order (temporal index slowest, width fastest)."""
    return {(f, i, j): encode(x[:, :, axes[0].span(f), axes[1].span(i), axes[2].span(j)])
            for f in range(axes[0].count) for i in range(axes[1].count) for j in range(axes[2].count)}


def blend_latent_tiles(raw: dict, axes: List[EncodeAxis], in_place: bool = True) -> torch.Tensor:
    """`in_place=True`: the reference's chain — every tile against the CURRENT (already blended) temporal, upper and left neighbour, in
    that order.  `in_place=False`: against the RAW neighbours, the rule of `tiled_decode`, kept for comparison.  Crop, concatenation."""
    at, ah, aw = axes
    cur = dict(raw)
    src = cur if in_place else raw
    for f in range(at.count):
        for i in range(ah.count):
            for j in range(aw.count):
                tile = raw[f, i, j]
                if f > 0:
                    tile = blend(src[f - 1, i, j], tile, 2, at.extent)
                if i > 0:
                    tile = blend(src[f, i - 1, j], tile, 3, ah.extent)
                if j > 0:
                    tile = blend(src[f, i, j - 1], tile, 4, aw.extent)
                cur[f, i, j] = tile
    frames = []
    for f in range(at.count):
        rows = []
        for i in range(ah.count):
            rows.append(torch.cat([cur[f, i, j][:, :, :at.limit, :ah.limit, :aw.limit] for j in range(aw.count)], dim=4))
        frames.append(torch.cat(rows, dim=3))
    return torch.cat(frames, dim=2)


def tiled_encode(encode, x: torch.Tensor, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length=16,
                 spatial_tile_overlap_factor=0.25, temporal_tile_overlap_factor=0, allow_spatial_tiling=False, ds=(4, 8, 8),
                 return_tiles: bool = False):
    """`ViTVAE.tiled_encode_3d` -> `TileProcessor.tiled_encode` with any tile encoder behind it."""
    if not allow_spatial_tiling:
        tile_sample_min_height = tile_sample_min_width = 100000
    axes = encode_axes(x.shape, (tile_sample_min_length, tile_sample_min_height, tile_sample_min_width), spatial_tile_overlap_factor,
                       temporal_tile_overlap_factor, ds)
    raw = encode_tiles(encode, x, axes)
    out = blend_latent_tiles(raw, axes)
    return (out, raw, axes) if return_tiles else out


def tile_case_kwargs(name: str) -> dict:
    _, (tl, th, tw), fs, ft, _, _, _ = TILE_CASES[name]
    return dict(tile_sample_min_length=tl, tile_sample_min_height=th, tile_sample_min_width=tw, spatial_tile_overlap_factor=fs,
                temporal_tile_overlap_factor=ft, allow_spatial_tiling=True)


def tile_case_axes(name: str) -> List[EncodeAxis]:
    shape, tile_px, fs, ft, _, _, _ = TILE_CASES[name]
    return encode_axes(shape, tile_px, fs, ft)


def load_raw_latent_tiles(fx: dict, axes: List[EncodeAxis]) -> dict:
    keys = [(f, i, j) for f in range(axes[0].count) for i in range(axes[1].count) for j in range(axes[2].count)]
    return {key: fx[f"tile_{k}"] for k, key in enumerate(keys)}

"""Shared by the MAGI tiled chunk decode tests and tools/gen_golden_magi_tiles.py: the fixtures' geometries and a plain-torch restatement
of `ViTVAE.tiled_decode_3d` -> `TileProcessor.tiled_decode` (inferix/models/magi/vae/vae_model.py:179-219,
inferix/distributed/parallelism/tile_parallel.py:348-448) with any tile decoder behind it.  On bf16 tensors it evaluates the reference's
eager op chain (each blend `bf16(bf16(a w1) + bf16(b w2))`, the weights Python floats applied at fp32 precision), so it equals the
reference-generated fixtures tests/golden/magi_tiles_*.npz bit for bit; on float32 tensors it is the exact-arithmetic evaluation the
measured-noise rule takes its floor from.  It runs on whatever device its tensors are on.  Nothing here imports oracle/, the reference or
inferix_amd.

`uint8_frames` restates the tail of `VaeHelper.decode` (inferix/pipeline/magi/video_process.py:195-199) as its four torch operators; that
module does not import without flash-attn, so this part is restated only, not reference-generated."""
from __future__ import annotations

from typing import Callable, List, Tuple

import torch

import magi_vit_util as U

# name -> (batch, latent shape, (tile length, height, width) in pixels, spatial overlap, temporal overlap, input seed, output shape)
WEIGHT_SEED = 4100           # the tiny decoder of magi_vit_util.TINY
CASES = {
    # 3 x 2 spatial grid, a 1-latent edge row, a T == 1 tile behind a full one (9 frames, not 12)
    "magi_tiles_a": (1, (3, 7, 5), (8, 32, 32), 0.25, 0.0, 21, (9, 56, 40)),
    # batch 2, temporal blend, e' = 1 against a one-frame tile, corner pixels blended three times
    "magi_tiles_b": (2, (3, 7, 5), (8, 32, 32), 0.25, 0.5, 22, (9, 56, 40)),
    # extent 24 (weights exact in no binary format), a 16-px edge tile narrower than the extent, 289-token tiles on a resized table
    "magi_tiles_c": (1, (3, 14, 11), (8, 96, 96), 0.25, 0.0, 23, (9, 112, 88)),
    # different height / width tiles, temporal extent 4 with limit 12
    "magi_tiles_d": (1, (5, 7, 11), (16, 32, 96), 0.25, 0.25, 24, (20, 56, 88)),
}


def case_kwargs(name: str) -> dict:
    _, _, (tl, th, tw), fs, ft, _, _ = CASES[name]
    return dict(tile_sample_min_length=tl, tile_sample_min_height=th, tile_sample_min_width=tw, spatial_tile_overlap_factor=fs,
                temporal_tile_overlap_factor=ft, allow_spatial_tiling=True)


def case_input(name: str, dtype=U.BF) -> torch.Tensor:
    batch, latent, _, _, _, seed, _ = CASES[name]
    return U.make_input(U.TINY, seed, batch, latent, dtype)


def tiny_decode(W, cfg=U.TINY) -> Callable[[torch.Tensor], torch.Tensor]:
    """`ViTVAE.decode` (vae_model.py:290-308) over the restated decoder: one latent frame gives one pixel frame."""
    def decode(t: torch.Tensor) -> torch.Tensor:
        out = U.decoder_forward(W, cfg, t)
        return out[:, :, :1] if t.shape[2] == 1 else out
    return decode


class Axis:
    """One axis of the tiling: tile size and stride in latents, blend extent and kept limit in pixels, tile count."""

    def __init__(self, size: int, tile_px: int, overlap: float, ds: int):
        self.tl = tile_px // ds
        self.stride = int(self.tl * (1 - overlap))
        full = int(self.tl * ds)
        self.extent = int(full * overlap)
        self.limit = full - self.extent
        self.count = -(-size // self.stride)

    def span(self, k: int) -> slice:
        return slice(k * self.stride, k * self.stride + self.tl)


def axes_of(shape, tile_px: Tuple[int, int, int], spatial_overlap: float, temporal_overlap: float, ds: Tuple[int, int, int]) -> List[Axis]:
    return [Axis(shape[-3 + i], tile_px[i], (temporal_overlap, spatial_overlap, spatial_overlap)[i], ds[i]) for i in range(3)]


def decode_tiles(decode, z: torch.Tensor, axes: List[Axis]):
    """Raw tile outputs keyed by (it, ih, iw), decoded in the reference's order (temporal index slowest, width fastest)."""
    raw = {}
    for it in range(axes[0].count):
        for ih in range(axes[1].count):
            for iw in range(axes[2].count):
                raw[it, ih, iw] = decode(z[:, :, axes[0].span(it), axes[1].span(ih), axes[2].span(iw)])
    return raw


def load_raw_tiles(name: str, axes: List[Axis]) -> dict:
    """The raw tile outputs of the reference's own `decode` calls (`<name>_raw.npz`), keyed like `decode_tiles` keys them."""
    fx = U.load_fixture(name + "_raw")
    keys = [(it, ih, iw) for it in range(axes[0].count) for ih in range(axes[1].count) for iw in range(axes[2].count)]
    assert len(fx) == len(keys)
    return {key: fx[f"tile_{k}"] for k, key in enumerate(keys)}


def case_axes(name: str) -> List[Axis]:
    _, latent, tile_px, fs, ft, _, _ = CASES[name]
    return axes_of(latent, tile_px, fs, ft, (4, 8, 8))


def _weighted(t: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """tensor x Python float as torch evaluates it: the product at fp32 precision, one rounding to the tensor's dtype."""
    return (t.float() * w).to(t.dtype)


def blend(a: torch.Tensor, b: torch.Tensor, dim: int, extent: int) -> torch.Tensor:
    """b with its first e' = min(len a, len b, extent) positions along `dim` mixed with the last e' of a: position p gets
    a (1 - p / e') + b (p / e'), quotient and difference in double as Python floats are, then cast to fp32."""
    e = min(a.shape[dim], b.shape[dim], extent)
    if e == 0:
        return b
    q = torch.arange(e, dtype=torch.float64) / e
    view = [1] * b.dim()
    view[dim] = e
    w1, w2 = (1.0 - q).float().view(view).to(b.device), q.float().view(view).to(b.device)
    head = _weighted(a.narrow(dim, a.shape[dim] - e, e), w1) + _weighted(b.narrow(dim, 0, e), w2)
    return torch.cat((head, b.narrow(dim, e, b.shape[dim] - e)), dim=dim)


def blend_tiles(raw: dict, axes: List[Axis]) -> torch.Tensor:
    """Every tile against its RAW temporal, upper and left neighbour in that order, cropped to the limits, concatenated."""
    at, ah, aw = axes
    frames = []
    for it in range(at.count):
        rows = []
        for ih in range(ah.count):
            row = []
            for iw in range(aw.count):
                tile = raw[it, ih, iw]
                if it > 0:
                    tile = blend(raw[it - 1, ih, iw], tile, 2, at.extent)
                if ih > 0:
                    tile = blend(raw[it, ih - 1, iw], tile, 3, ah.extent)
                if iw > 0:
                    tile = blend(raw[it, ih, iw - 1], tile, 4, aw.extent)
                row.append(tile[:, :, :at.limit, :ah.limit, :aw.limit])
            rows.append(torch.cat(row, dim=4))
        frames.append(torch.cat(rows, dim=3))
    return torch.cat(frames, dim=2)


def tiled_decode_restated(decode, z: torch.Tensor, tile_sample_min_height=256, tile_sample_min_width=256, tile_sample_min_length=16,
                          spatial_tile_overlap_factor=0.25, temporal_tile_overlap_factor=0, allow_spatial_tiling=False,
                          ds: Tuple[int, int, int] = (4, 8, 8), return_tiles: bool = False):
    if not allow_spatial_tiling:
        tile_sample_min_height = tile_sample_min_width = 100000
    axes = axes_of(z.shape, (tile_sample_min_length, tile_sample_min_height, tile_sample_min_width), spatial_tile_overlap_factor,
                   temporal_tile_overlap_factor, ds)
    raw = decode_tiles(decode, z, axes)
    out = blend_tiles(raw, axes)
    return (out, raw, axes) if return_tiles else out


def uint8_frames(x: torch.Tensor) -> torch.Tensor:
    """'b c t h w -> (b t) c h w', x 127.5 + 127.5, clamp(0, 255), truncation to uint8."""
    N, C, T, H, W = x.shape
    f = x.permute(0, 2, 1, 3, 4).reshape(N * T, C, H, W)
    f = (f * 127.5) + 127.5
    return f.clamp(0, 255).type(torch.uint8)

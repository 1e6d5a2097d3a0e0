"""The tile plan of MAGI's chunk decode: `TileProcessor.tiled_decode` (inferix/distributed/parallelism/tile_parallel.py:348-448) as
integers.  `plan_tiles` evaluates the reference's formulas as they are written there (the `int(...)` truncations included) and returns
the tile list in the reference's order (temporal index slowest, width index fastest), every tile's decoded extent with the T == 1 rule
of `ViTVAE.decode`, the blend extents, the crop limits and the output shape.  `blend_table` lays the plan out as the int64 descriptor
table of `ifx_vit_tile_blend` (include/inferix_hip.h).  Nothing here touches a device.

Per axis, with the tile size in latents `tl = tile_sample_min // ds`, the downsample factor `ds` and the overlap factor `f`:
    stride  s = int(tl (1 - f)) latents        blend extent  e = int(int(tl ds) f) pixels        limit  lim = tl ds - e pixels
    tiles   n = ceil(size / s), tile k covers latents [k s, min(k s + tl, size))
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Dict, List, Tuple

import torch


@dataclasses.dataclass(frozen=True)
class AxisPlan:
    size: int                      # latents
    tile: int                      # tl
    stride: int                    # s
    blend: int                     # e, pixels
    limit: int                     # lim, pixels
    spans: Tuple[Tuple[int, int], ...]      # latent [begin, end) of tile k
    extents: Tuple[int, ...]       # decoded pixels of tile k
    starts: Tuple[int, ...]        # output start of tile k: the kept extents of its predecessors

    @property
    def count(self) -> int:
        return len(self.spans)

    @property
    def out(self) -> int:
        return self.starts[-1] + min(self.extents[-1], self.limit)

    def blend_extent(self, k: int) -> int:
        """e' of tile k against its predecessor: the reference's `min(a.shape, b.shape, blend_extent)`; 0 for the first tile."""
        return min(self.extents[k - 1], self.extents[k], self.blend) if k > 0 else 0


@dataclasses.dataclass(frozen=True)
class TilePlan:
    axes: Tuple[AxisPlan, AxisPlan, AxisPlan]        # t, h, w
    tiles: Tuple[Tuple[int, int, int], ...]          # (it, ih, iw) in the reference's order

    @property
    def grid(self) -> Tuple[int, int, int]:
        return tuple(a.count for a in self.axes)

    @property
    def out_shape(self) -> Tuple[int, int, int]:
        return tuple(a.out for a in self.axes)

    def latent_span(self, idx) -> Tuple[Tuple[int, int], ...]:
        return tuple(a.spans[k] for a, k in zip(self.axes, idx))

    def latent_shape(self, idx) -> Tuple[int, int, int]:
        return tuple(e - b for b, e in self.latent_span(idx))

    def decoded_shape(self, idx) -> Tuple[int, int, int]:
        return tuple(a.extents[k] for a, k in zip(self.axes, idx))

    def groups(self) -> Dict[Tuple[int, int, int], List[int]]:
        """latent shape -> positions in `tiles` of the tiles that have it (insertion order: first appearance)."""
        g: Dict[Tuple[int, int, int], List[int]] = {}
        for i, idx in enumerate(self.tiles):
            g.setdefault(self.latent_shape(idx), []).append(i)
        return g

    def traffic_elements(self, batch: int) -> Tuple[int, int]:
        """(output pixels, tile values read) of one blend pass: one read per own pixel and one per active blend."""
        reads = 0
        for it, ih, iw in self.tiles:
            kept = [min(a.extents[k], a.limit) for a, k in zip(self.axes, (it, ih, iw))]
            own = kept[0] * kept[1] * kept[2]
            reads += own
            for ax, k in enumerate((it, ih, iw)):
                e = min(self.axes[ax].blend_extent(k), kept[ax])
                reads += own // kept[ax] * e
        pixels = batch * 3 * self.out_shape[0] * self.out_shape[1] * self.out_shape[2]
        return pixels, batch * 3 * reads


def _axis(name: str, size: int, tile_sample_min: int, overlap: float, ds: int, single_frame_rule: bool) -> AxisPlan:
    tl = tile_sample_min // ds
    if size < 1 or tl < 1:
        raise ValueError(f"plan_tiles: {name}: size {size} latents, tile {tile_sample_min} px / {ds} = {tl} latents")
    s = int(tl * (1 - overlap))
    if s < 1:
        raise ValueError(f"plan_tiles: {name}: overlap factor {overlap} leaves a stride of {s} latents for tiles of {tl}")
    real = int(tl * ds)
    e = int(real * overlap)
    lim = real - e
    n = (size + s - 1) // s
    if n > 1 and lim != s * ds:
        raise NotImplementedError(
            f"plan_tiles: {name}: tiles of {tl} latents ({real} px) with overlap factor {overlap} advance by {s} latents = {s * ds} px but "
            f"keep {lim} px each (blend extent {e}); the reference's concatenation does not line up with its input there")
    spans = tuple((k * s, min(k * s + tl, size)) for k in range(n))
    extents = tuple(1 if single_frame_rule and e_ - b == 1 else (e_ - b) * ds for b, e_ in spans)
    starts, at = [], 0
    for x in extents:
        starts.append(at)
        at += min(x, lim)
    return AxisPlan(size, tl, s, e, lim, spans, extents, tuple(starts))


def plan_tiles(latent_shape, tile_sample_min_length: int = 16, tile_sample_min_height: int = 256, tile_sample_min_width: int = 256,
               spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, spatial_downsample_factor: int = 8,
               temporal_downsample_factor: int = 4) -> TilePlan:
    """The plan for latents of `latent_shape` = (T, H, W) (the last three entries of a longer shape)."""
    T, H, W = (int(v) for v in tuple(latent_shape)[-3:])
    axes = (_axis("length", T, tile_sample_min_length, temporal_tile_overlap_factor, temporal_downsample_factor, True),
            _axis("height", H, tile_sample_min_height, spatial_tile_overlap_factor, spatial_downsample_factor, False),
            _axis("width", W, tile_sample_min_width, spatial_tile_overlap_factor, spatial_downsample_factor, False))
    nt, nh, nw = (a.count for a in axes)
    tiles = tuple((it, ih, iw) for it in range(nt) for ih in range(nh) for iw in range(nw))
    return TilePlan(axes, tiles)


@dataclasses.dataclass(frozen=True)
class BlendTable:
    """The descriptor of one `ifx_vit_tile_blend` launch as the host knows it; `hip_ops.vit_tile_blend` uploads `words` once."""
    words: Tuple[int, ...]         # the int64 table
    offsets: Tuple[int, ...]       # arena element offset per tile
    arena_elements: int            # the arena has to hold at least this many bf16 values
    batch: int
    grid: Tuple[int, int, int]
    out_shape: Tuple[int, int, int]
    blends: Tuple[int, int, int]
    limits: Tuple[int, int, int]
    vec_x: bool                    # every x extent, x start and offset is a multiple of 8
    frame_pitch: Tuple[int, ...] = ()      # per temporal index: frames a tile's storage holds

    def tensor(self, device) -> torch.Tensor:
        return torch.tensor(self.words, dtype=torch.int64, device=device)


def _weight_word(p: int, e: int) -> int:
    """fp32(1 - p / e) in the low half and fp32(p / e) in the high half of one int64 word (both expressions in double first)."""
    return struct.unpack("<q", struct.pack("<ff", 1 - p / e, p / e))[0]


def blend_table(batch: int, extents, starts, blends, limits, out_shape, offsets=None, frame_pitch=None, align: int = 8) -> BlendTable:
    """`extents` / `starts`: per axis (t, h, w) the decoded extent and the output start of every tile index; `frame_pitch`: per temporal
    index the frames a tile's storage holds (default: its extent).  Without `offsets` the tiles are packed in the reference's order,
    each `[batch, 3, P_k, H_k, W_k]`, starts rounded up to `align` elements."""
    nt, nh, nw = (len(e) for e in extents)
    frame_pitch = tuple(extents[0]) if frame_pitch is None else tuple(int(p) for p in frame_pitch)
    assert len(frame_pitch) == nt and all(p >= e for p, e in zip(frame_pitch, extents[0]))
    sizes = [batch * 3 * frame_pitch[it] * extents[1][ih] * extents[2][iw] for it in range(nt) for ih in range(nh) for iw in range(nw)]
    if offsets is None:
        offsets, at = [], 0
        for n in sizes:
            offsets.append(at)
            at += -(-n // align) * align
    offsets = tuple(int(o) for o in offsets)
    assert len(offsets) == len(sizes) and all(len(s) == len(e) for s, e in zip(starts, extents))
    words = list(offsets)
    for e, s in zip(extents, starts):
        words += list(e) + list(s)
    words += list(frame_pitch)
    for e, blend in zip(extents, blends):          # [tile index][position] -> (w1, w2) as the reference's Python floats, cast to fp32
        for k in range(len(e)):
            ek = min(e[k - 1], e[k], blend) if k > 0 else 0
            words += [_weight_word(p, ek) if p < ek else 0 for p in range(blend)]
    vec = all(v % 8 == 0 for v in tuple(extents[2]) + tuple(starts[2]) + offsets) and out_shape[2] % 8 == 0 and blends[2] % 8 == 0
    return BlendTable(tuple(int(w) for w in words), offsets, max(o + n for o, n in zip(offsets, sizes)), batch, (nt, nh, nw),
                      tuple(out_shape), tuple(blends), tuple(limits), vec, frame_pitch)


def plan_blend_table(plan: TilePlan, batch: int, offsets=None, frame_pitch=None) -> BlendTable:
    return blend_table(batch, [a.extents for a in plan.axes], [a.starts for a in plan.axes], [a.blend for a in plan.axes],
                       [a.limit for a in plan.axes], plan.out_shape, offsets=offsets, frame_pitch=frame_pitch)


# ---- the encode side: `TileProcessor.tiled_encode` (tile_parallel.py:254-346) -----------------------------------------------------------
# The same dataclasses with the units the reference uses THERE: the input is cut in pixels, the blend runs on latents.  Per axis, with
# the tile in pixels `tp = tile_sample_min`, `tl = tp // ds` latents and the overlap factor `f` (:255-269):
#     stride  s = int(tp (1 - f)) PIXELS        blend extent  e = int(tl f) LATENTS        limit  lim = tl - e LATENTS
#     tiles   n = ceil(size / s), tile k covers pixels [k s, min(k s + tp, size)) and encodes to floor(pixels / ds) latents
# so in an encode plan `AxisPlan.size`, `.stride` and `.spans` are pixels, `.tile`, `.blend`, `.limit`, `.extents`, `.starts` latents, and
# `TilePlan.groups()` groups the tiles by PIXEL shape.
def _encode_axis(name: str, size: int, tile_sample_min: int, overlap: float, ds: int, single_frame_rule: bool) -> AxisPlan:
    tl = tile_sample_min // ds
    if size < 1 or tl < 1:
        raise ValueError(f"plan_encode_tiles: {name}: size {size} px, tile {tile_sample_min} px / {ds} = {tl} latents")
    s = int(tile_sample_min * (1 - overlap))
    if s < 1:
        raise ValueError(f"plan_encode_tiles: {name}: overlap factor {overlap} leaves a stride of {s} px for tiles of {tile_sample_min}")
    e = int(tl * overlap)
    lim = tl - e
    n = (size + s - 1) // s
    if n > 1 and lim * ds != s:
        raise NotImplementedError(
            f"plan_encode_tiles: {name}: tiles of {tile_sample_min} px ({tl} latents) with overlap factor {overlap} advance by {s} px but keep "
            f"{lim} latents = {lim * ds} px each (blend extent {e}); the reference's concatenation does not line up with its input there")
    spans = tuple((k * s, min(k * s + tile_sample_min, size)) for k in range(n))
    extents = []
    for b, e_ in spans:
        px = e_ - b
        if single_frame_rule and px == 1 and ds > 1:      # `ViTVAE.encode`: one frame is expanded to 4 and the first latent frame is kept
            if 4 // ds < 1:
                raise ValueError(f"plan_encode_tiles: {name}: a single frame expands to 4, less than one patch of {ds}")
            extents.append(1)
        elif px // ds < 1:
            raise ValueError(f"plan_encode_tiles: {name}: tile [{b}, {e_}) holds {px} px, less than one patch of {ds} (the reference's "
                             "patch convolution raises on it)")
        else:
            extents.append(px // ds)
    starts, at = [], 0
    for x in extents:
        starts.append(at)
        at += min(x, lim)
    return AxisPlan(size, tl, s, e, lim, spans, tuple(extents), tuple(starts))


def plan_encode_tiles(video_shape, tile_sample_min_length: int = 16, tile_sample_min_height: int = 256, tile_sample_min_width: int = 256,
                      spatial_tile_overlap_factor: float = 0.25, temporal_tile_overlap_factor: float = 0, spatial_downsample_factor: int = 8,
                      temporal_downsample_factor: int = 4) -> TilePlan:
    """The encode plan for a video of `video_shape` = (T, H, W) pixels (the last three entries of a longer shape)."""
    T, H, W = (int(v) for v in tuple(video_shape)[-3:])
    axes = (_encode_axis("length", T, tile_sample_min_length, temporal_tile_overlap_factor, temporal_downsample_factor, True),
            _encode_axis("height", H, tile_sample_min_height, spatial_tile_overlap_factor, spatial_downsample_factor, False),
            _encode_axis("width", W, tile_sample_min_width, spatial_tile_overlap_factor, spatial_downsample_factor, False))
    nt, nh, nw = (a.count for a in axes)
    return TilePlan(axes, tuple((it, ih, iw) for it in range(nt) for ih in range(nh) for iw in range(nw)))


@dataclasses.dataclass(frozen=True)
class LatentBlendTable:
    """The descriptor of one `ifx_vit_latent_blend` call as the host knows it."""
    words: Tuple[int, ...]         # the int64 table
    offsets: Tuple[int, ...]       # arena element offset per tile
    arena_elements: int
    planes: int                    # samples x channels
    grid: Tuple[int, int, int]
    blends: Tuple[int, int, int]
    diagonal_max: Tuple[int, ...]  # per anti-diagonal the largest planes x T x H x W of its tiles

    def tensor(self, device) -> torch.Tensor:
        return torch.tensor(self.words, dtype=torch.int64, device=device)


def latent_blend_table(planes: int, extents, blends, offsets=None) -> LatentBlendTable:
    """`extents`: per axis (t, h, w) the latent extent of every tile index; `blends`: the three blend extents in latents.  Without
    `offsets` the tiles are packed in the reference's order, each `[planes, T_k, H_k, W_k]`."""
    nt, nh, nw = (len(e) for e in extents)
    idx = [(f, i, j) for f in range(nt) for i in range(nh) for j in range(nw)]
    sizes = [planes * extents[0][f] * extents[1][i] * extents[2][j] for f, i, j in idx]
    if offsets is None:
        offsets, at = [], 0
        for n in sizes:
            offsets.append(at)
            at += n
    offsets = tuple(int(o) for o in offsets)
    assert len(offsets) == len(sizes)
    words = list(offsets)
    for e in extents:
        words += list(e)
    for e, blend in zip(extents, blends):
        for k in range(len(e)):
            ek = min(e[k - 1], e[k], blend) if k > 0 else 0
            words += [_weight_word(p, ek) if p < ek else 0 for p in range(blend)]
    order = sorted(range(len(idx)), key=lambda k: (sum(idx[k]), k))
    words += order
    diagonal_max = tuple(max(sizes[k] for k in order if sum(idx[k]) == d) for d in range(nt + nh + nw - 2))
    return LatentBlendTable(tuple(int(w) for w in words), offsets, max(o + n for o, n in zip(offsets, sizes)), planes, (nt, nh, nw),
                            tuple(int(b) for b in blends), diagonal_max)


def plan_latent_blend_table(plan: TilePlan, planes: int, offsets=None) -> LatentBlendTable:
    return latent_blend_table(planes, [a.extents for a in plan.axes], [a.blend for a in plan.axes], offsets=offsets)

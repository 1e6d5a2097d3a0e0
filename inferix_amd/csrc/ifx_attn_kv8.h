// Host-side launch plan of the 8-bit self-attention kernel (ifx_attn_kv8.hip): tile sizes, the ring, the LDS layout of a slot and the
// per-XCD raster, shared by the launcher, the kernel (the constants) and ifx_attn_kv8_plan.  No GPU call.
#pragma once
#include "../../include/inferix_hip_kv8.h"
#include "../../include/inferix_hip_kv8_split.h"
#include "../../include/inferix_hip_kv8_ring.h"
#include "../../include/inferix_hip_kv8_ring_split.h"

namespace ifx {
namespace kv8 {

constexpr int kRows = 256;                 // query rows per workgroup: 8 waves x one 32-row MFMA block
constexpr int kKeys = 64;                  // keys per tile: two 32-key score blocks = ONE K = 64 step of the PV product
constexpr int kRing = 3;                   // slots: tile t is computed while t + 1 is being transposed and t + 2 is in flight
constexpr int kKTile = kKeys * 128;        // K tile as it lies in the cache: 64 rows x 128 B, 16-byte chunks XOR-swizzled by (row >> 1) & 7
// V tile TRANSPOSED: 128 channel rows x 64 key bytes, 16 B of padding after every 4 rows (the transposing stores of one wave go to
// rows 4 c + e, c = 0 .. 31: without the padding all of them would fall into one bank)
constexpr int kVtTile = 128 * kKeys + 32 * 16;
constexpr int kSlot = kKTile + kVtTile;
constexpr int kLds = kRing * kSlot;

inline bool plan(int q_rows, int heads, int kv_start, int kv_len, ifx_kv8_plan* p) {
  if (!p || q_rows <= 0 || heads <= 0 || kv_start < 0 || kv_len <= kv_start) return false;
  p->row_tiles = (q_rows + kRows - 1) / kRows;
  p->key_tiles = (kv_len - kv_start + kKeys - 1) / kKeys;
  p->per_xcd = (p->row_tiles * heads + 7) / 8;
  p->grid = 8 * p->per_xcd;
  p->ring = kRing;
  p->lds_bytes = kLds;
  return true;
}

// ---- the split-key launch (include/inferix_hip_kv8_split.h): the key tiles of a (head, row tile) group are dealt to `chunks`
// workgroups, which leave fp32 partials in a workspace; the last of a group to arrive merges them in chunk order.
// Workspace: [counter_bytes] int32 arrivals per group, then fp32 [chunk][head][row_tile][wave 0 .. 7][kPartWave]: the 32 rows of a wave
// as the wave holds them.  Lane (n, h) = (lane & 31, lane >> 5) has channels 32 db + 8 g + 4 h + e of row n in register 4 g + e of
// accumulator db; piece j = 4 db + g of the block is those four floats of all 64 lanes ([j][lane][4]: one store instruction writes 1 KiB
// in a row), and piece 16 is {m, l, 0, 0} of rows n = 0 .. 31, stored by lane half 0.  Every store is a whole 16-byte piece, the merge's
// lane reads back exactly the pieces it would have written, and rows past q_rows are neither written nor read.
constexpr int kMaxSplits = IFX_KV8_SPLIT_MAX;
constexpr int kPartWords = IFX_KV8_SPLIT_ROW_WORDS;
constexpr int kPartWave = 32 * kPartWords;      // words of a wave's block: 16 pieces of 64 lanes x 4 and one of 32 x 4
constexpr int kSplitCus = 256;             // the chooser fills at most this many workgroups ...
constexpr int kSplitFull = 128;            // ... and leaves a launch alone that has more groups than this

// chunks the chooser picks for a shape: the largest s <= 16 with groups * s <= 256 and key_tiles / s >= min_tiles, or 1
inline int auto_splits(int row_tiles, int heads, int key_tiles, int min_tiles) {
  const long long groups = (long long)row_tiles * heads;
  if (groups > kSplitFull) return 1;
  int s = (int)(kSplitCus / groups) < kMaxSplits ? (int)(kSplitCus / groups) : kMaxSplits;
  while (s > 1 && key_tiles / s < min_tiles) --s;
  return s;
}

// first tile of chunk c when `tiles` are dealt to `chunks` (the first tiles % chunks chunks hold one more)
inline int chunk_tile0(int tiles, int chunks, int c) { return c * (tiles / chunks) + (c < tiles % chunks ? c : tiles % chunks); }

// num_splits 0 = choose with min_tiles
inline bool split_plan(int q_rows, int heads, int kv_start, int kv_len, int num_splits, int min_tiles, ifx_kv8_split_plan* p) {
  ifx_kv8_plan b;
  if (!p || num_splits < 0 || num_splits > kMaxSplits || !plan(q_rows, heads, kv_start, kv_len, &b)) return false;
  *p = ifx_kv8_split_plan{};
  if (num_splits == 0) num_splits = auto_splits(b.row_tiles, heads, b.key_tiles, min_tiles);
  const int chunks = num_splits < b.key_tiles ? num_splits : b.key_tiles;
  const long long groups = (long long)b.row_tiles * heads;
  p->chunks = chunks, p->row_tiles = b.row_tiles, p->key_tiles = b.key_tiles, p->lds_bytes = kLds;
  for (int c = 0; c < chunks; ++c) p->tiles_per_chunk[c] = chunk_tile0(b.key_tiles, chunks, c + 1) - chunk_tile0(b.key_tiles, chunks, c);
  if (chunks == 1) {      // ifx_attn_fwd_kv8's own raster
    p->grid = b.grid;
    for (int x = 0; x < 8; ++x) {
      const long long left = groups - (long long)x * b.per_xcd;
      p->xcd_groups[x] = (int)(left < 0 ? 0 : left < b.per_xcd ? left : b.per_xcd);
    }
    return true;
  }
  for (int x = 0; x < 8; ++x) p->xcd_groups[x] = (int)((x + 1) * groups / 8 - x * groups / 8);
  p->grid = 8 * (int)((groups + 7) / 8) * chunks;
  p->counter_bytes = (int)((groups * 4 + 255) / 256 * 256);
  p->workspace_bytes = p->counter_bytes + (long long)chunks * heads * b.row_tiles * kRows * kPartWords * 4;
  return true;
}

// ---- the grouped launch (include/inferix_hip_kv8_ring.h): slots [0, kv_len) in groups of `tokens` slots that share a V scale.  The
// key tiles are counted per group (tile t is tile t % tpg of group t / tpg and starts at slot g * tokens + 64 j), so that no tile holds
// rows of two scales; the keys of a group's last tile that belong to the next group are masked by index.
inline bool grouped_plan(int q_rows, int heads, int tokens, int kv_len, ifx_kv8_grouped_plan* p) {
  ifx_kv8_plan b;
  if (!p || tokens <= 0 || !plan(q_rows, heads, 0, kv_len, &b)) return false;
  p->row_tiles = b.row_tiles, p->per_xcd = b.per_xcd, p->grid = b.grid, p->ring = b.ring, p->lds_bytes = b.lds_bytes;
  p->tiles_per_group = (tokens + kKeys - 1) / kKeys;
  p->groups = (kv_len + tokens - 1) / tokens;
  p->key_tiles = (kv_len / tokens) * p->tiles_per_group + (kv_len % tokens + kKeys - 1) / kKeys;
  return true;
}

// ---- the grouped split-key launch (include/inferix_hip_kv8_ring_split.h): the tiles of the grouped walk dealt to chunks as split_plan
// deals the flat launch's, behind the same raster and over the same workspace.  A chunk is described by where its first tile stands in
// the walk (group, tile in group), so that the kernel starts its cursors there without dividing, and by the group of its last tile,
// whose scale is the unit of its partial O.
static_assert(IFX_KV8_GROUPED_SPLIT_MAX == kMaxSplits && IFX_KV8_GROUPED_SPLIT_ROW_WORDS == kPartWords, "one workspace layout for both split launches");
constexpr int kXcdCus = 32;               // the chooser gives no XCD more workgroups than this

// chunks the chooser picks: the largest s <= 16 with key_tiles / s >= min_tiles and ceil(groups / 8) * s <= 32, or 1
inline int grouped_auto_splits(int row_tiles, int heads, int key_tiles, int min_tiles) {
  const long long groups = (long long)row_tiles * heads;
  if (groups > kSplitFull) return 1;
  int s = kMaxSplits;
  while (s > 1 && (key_tiles / s < min_tiles || (groups + 7) / 8 * s > kXcdCus)) --s;
  return s;
}

// num_splits 0 = choose with min_tiles
inline bool grouped_split_plan(int q_rows, int heads, int tokens, int kv_len, int num_splits, int min_tiles, ifx_kv8_grouped_split_plan* p) {
  ifx_kv8_grouped_plan b;
  if (!p || num_splits < 0 || num_splits > kMaxSplits || !grouped_plan(q_rows, heads, tokens, kv_len, &b)) return false;
  *p = ifx_kv8_grouped_split_plan{};
  if (num_splits == 0) num_splits = grouped_auto_splits(b.row_tiles, heads, b.key_tiles, min_tiles);
  const int chunks = num_splits < b.key_tiles ? num_splits : b.key_tiles, tpg = b.tiles_per_group;
  const long long groups = (long long)b.row_tiles * heads;
  p->chunks = chunks, p->row_tiles = b.row_tiles, p->key_tiles = b.key_tiles, p->tiles_per_group = tpg, p->key_groups = b.groups;
  p->lds_bytes = kLds;
  for (int c = 0; c < chunks; ++c) {       // (only the walk's last group can hold fewer than tpg tiles, so t / tpg is every tile's group)
    const int t0 = chunk_tile0(b.key_tiles, chunks, c), t1 = chunk_tile0(b.key_tiles, chunks, c + 1);
    p->tiles_per_chunk[c] = t1 - t0, p->first_group[c] = t0 / tpg, p->first_tile[c] = t0 % tpg, p->last_group[c] = (t1 - 1) / tpg;
  }
  if (chunks == 1) {      // ifx_attn_fwd_kv8_grouped's own raster
    p->grid = b.grid;
    for (int x = 0; x < 8; ++x) {
      const long long left = groups - (long long)x * b.per_xcd;
      p->xcd_groups[x] = (int)(left < 0 ? 0 : left < b.per_xcd ? left : b.per_xcd);
    }
    return true;
  }
  for (int x = 0; x < 8; ++x) p->xcd_groups[x] = (int)((x + 1) * groups / 8 - x * groups / 8);
  p->grid = 8 * (int)((groups + 7) / 8) * chunks;
  p->counter_bytes = (int)((groups * 4 + 255) / 256 * 256);
  p->workspace_bytes = p->counter_bytes + (long long)chunks * heads * b.row_tiles * kRows * kPartWords * 4;
  return true;
}

}  // namespace kv8
}  // namespace ifx

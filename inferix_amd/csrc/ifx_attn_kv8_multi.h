// ifx_attn_fwd_kv8_multi / ifx_rmsnorm_rope_kv8_append_multi: the kernels' by-value argument structs and the attention launch's work
// split (host arithmetic, no GPU call), shared by the launcher, the kernel and ifx_attn_kv8_multi_plan.  The split is stated in
// include/inferix_hip_kv8_sessions.h; the single launch's constants and LDS layout are those of ifx_attn_kv8.h.
#pragma once
#include "../../include/inferix_hip_kv8_sessions.h"
#include "../../include/inferix_hip_kv8_ring_sessions.h"
#include "../../include/inferix_hip_kv8_magi.h"
#include "ifx_attn_kv8.h"
#include "ifx_rows.h"

namespace ifx {
namespace kv8 {

constexpr int kMultiItems = IFX_KV8_MULTI_MAX_ITEMS;
constexpr int kMultiStreams = IFX_KV8_MULTI_MAX_STREAMS;
constexpr int kXcds = 8;
// a raster word: local tile of the stream's first row tile << 12 | head << 3 | item.  Within an XCD's list the words ascend, so the
// prologue searches them as they are.
constexpr int kHeadBits = 9, kItemBits = 3, kTile0Shift = kHeadBits + kItemBits, kMaxTile0 = 1 << (32 - kTile0Shift);

// One item as the attention kernel reads it: what differs between the items' own single launches.
struct AttnKv8Item {
  const unsigned char* q;
  unsigned short* out;
  const unsigned char *k, *v;
  const float* v_scale;
  int ldq, ldo, q_rows, kv_start, kv_len, row_tiles;
};
struct AttnKv8MultiArgs {
  AttnKv8Item item[kMultiItems];       // in launch order (MultiPlan::order)
  unsigned stream[kMultiStreams];      // raster words, XCD 0's list first
  int xcd_first[kXcds + 1];
  int xcd_tiles[kXcds];
  int group, pitch;                    // heads / kv_heads; bytes of a cache row
};
static_assert(sizeof(AttnKv8MultiArgs) <= 4096, "the raster table travels in the kernel arguments");

// One item as the append kernel reads it.
struct Kv8AppendItem {
  const unsigned short* qkv;
  unsigned char *q8, *k, *v;
  const float* v_scale;
  RopeArgs ra;
  int ld, local_start;
};
struct Kv8AppendMultiArgs {
  Kv8AppendItem item[kMultiItems];
  int row0[kMultiItems + 1];           // rows [row0[i], row0[i + 1]) of the launch belong to item[i]
  const unsigned short *wq, *wk;
  int n_items, dim, head_dim;
  float eps;
};
static_assert(sizeof(Kv8AppendMultiArgs) <= 4096, "the item table travels in the kernel arguments");

struct MultiPlan {
  int n_streams, grid;
  int order[kMultiItems];              // order[i] = the caller's index of launch item i: longest key range first (stable)
  int xcd_first[kXcds + 1], xcd_tiles[kXcds];
  long long xcd_cost[kXcds];
  int item[kMultiStreams], head[kMultiStreams], tile0[kMultiStreams];      // per stream, in list order; item = launch position
};

// IFX_OK, IFX_EINVAL (bad shapes) or IFX_EUNSUP (the table does not hold the set); the caller words the error.
// `key_tiles`: the tiles a workgroup of item i walks along the keys where that is not ceil(keys / 64) — the grouped launch's per-group
// count (grouped_key_tiles below); nullptr = the flat count.
inline int plan_multi(const int* q_rows, const int* kv_start, const int* kv_len, int n, int heads, MultiPlan& p, const int* key_tiles = nullptr) {
  if (!q_rows || !kv_start || !kv_len || n < 1 || n > kMultiItems || heads <= 0) return IFX_EINVAL;
  for (int i = 0; i < n; ++i)
    if (q_rows[i] < 0 || kv_start[i] < 0 || kv_len[i] <= kv_start[i]) return IFX_EINVAL;
  if ((long long)n * heads > kMultiStreams || heads >= (1 << kHeadBits)) return IFX_EUNSUP;
  auto keys = [&](int i) { return key_tiles ? key_tiles[i] : (kv_len[i] - kv_start[i] + kKeys - 1) / kKeys; };
  auto rows = [&](int i) { return (q_rows[i] + kRows - 1) / kRows; };
  p = MultiPlan{};
  for (int i = 0; i < n; ++i) {
    int j = i;
    for (; j > 0 && kv_len[i] - kv_start[i] > kv_len[p.order[j - 1]] - kv_start[p.order[j - 1]]; --j) p.order[j] = p.order[j - 1];
    p.order[j] = i;
  }
  // streams in order of non-increasing cost (stable over launch position, head), each to the XCD with the least cost so far
  int s_item[kMultiStreams], s_head[kMultiStreams], s_xcd[kMultiStreams], ns = 0;
  for (int i = 0; i < n; ++i)
    for (int h = 0; h < heads && q_rows[p.order[i]] > 0; ++h) {
      const long long c = (long long)rows(p.order[i]) * keys(p.order[i]);
      int j = ns++;
      for (; j > 0 && c > (long long)rows(p.order[s_item[j - 1]]) * keys(p.order[s_item[j - 1]]); --j) s_item[j] = s_item[j - 1], s_head[j] = s_head[j - 1];
      s_item[j] = i, s_head[j] = h;
    }
  int count[kXcds] = {};
  for (int s = 0; s < ns; ++s) {
    int x = 0;
    for (int y = 1; y < kXcds; ++y)
      if (p.xcd_cost[y] < p.xcd_cost[x]) x = y;
    s_xcd[s] = x;
    p.xcd_cost[x] += (long long)rows(p.order[s_item[s]]) * keys(p.order[s_item[s]]);
    ++count[x];
  }
  for (int x = 0; x < kXcds; ++x) p.xcd_first[x + 1] = p.xcd_first[x] + count[x];
  // an XCD's list: longest key range first, ties in the order of assignment
  int fill[kXcds];
  for (int x = 0; x < kXcds; ++x) fill[x] = p.xcd_first[x];
  for (int s = 0; s < ns; ++s) {
    const int x = s_xcd[s];
    int j = fill[x]++;
    for (; j > p.xcd_first[x] && keys(p.order[s_item[s]]) > keys(p.order[p.item[j - 1]]); --j) p.item[j] = p.item[j - 1], p.head[j] = p.head[j - 1];
    p.item[j] = s_item[s], p.head[j] = s_head[s];
  }
  int most = 0;
  for (int x = 0; x < kXcds; ++x) {
    long long t = 0;
    for (int s = p.xcd_first[x]; s < p.xcd_first[x + 1]; ++s) {
      if (t >= kMaxTile0) return IFX_EUNSUP;
      p.tile0[s] = (int)t;
      t += rows(p.order[p.item[s]]);
    }
    if (t >= kMaxTile0) return IFX_EUNSUP;
    p.xcd_tiles[x] = (int)t;
    most = most > (int)t ? most : (int)t;
  }
  p.n_streams = ns;
  p.grid = kXcds * most;
  return IFX_OK;
}

// ---- the ring cache's launches (include/inferix_hip_kv8_ring_sessions.h)
static_assert(IFX_KV8_RING_MULTI_MAX_ITEMS == kMultiItems && IFX_KV8_RING_MULTI_MAX_STREAMS == kMultiStreams, "one raster word format");

// One item as the grouped attention kernel reads it: AttnKv8Item with the tiles of the item's walk in place of the first key.
struct AttnKv8GroupedItem {
  const unsigned char* q;
  unsigned short* out;
  const unsigned char *k, *v;
  const float* v_scale;                // the item's table [group][kv_head]
  int ldq, ldo, q_rows, kv_len, row_tiles, nt;
};
struct AttnKv8GroupedMultiArgs {
  AttnKv8GroupedItem item[kMultiItems];      // in launch order (MultiPlan::order)
  unsigned stream[kMultiStreams];
  int xcd_first[kXcds + 1];
  int xcd_tiles[kXcds];
  int group, pitch;                    // heads / kv_heads; bytes of a cache row
  int tokens, tpg, kv_heads;           // GroupWalk's launch-wide fields
};
static_assert(sizeof(AttnKv8GroupedMultiArgs) <= 4096, "the raster table travels in the kernel arguments");

// key tiles of ifx_attn_fwd_kv8_grouped's walk over slots [0, kv_len) in groups of `tokens` (grouped_plan's count)
inline int grouped_key_tiles(int tokens, int kv_len) {
  return (kv_len / tokens) * ((tokens + kKeys - 1) / kKeys) + (kv_len % tokens + kKeys - 1) / kKeys;
}

// plan_multi for the grouped launch: kv_start = 0 and the per-group tile count
inline int plan_grouped_multi(const int* q_rows, const int* kv_len, int n, int heads, int tokens, MultiPlan& p) {
  if (!q_rows || !kv_len || n < 1 || n > kMultiItems || tokens <= 0) return IFX_EINVAL;
  int zero[kMultiItems] = {}, tiles[kMultiItems];
  for (int i = 0; i < n; ++i) tiles[i] = kv_len[i] > 0 ? grouped_key_tiles(tokens, kv_len[i]) : 0;
  return plan_multi(q_rows, zero, kv_len, n, heads, p, tiles);
}

// One item as the ring append kernel reads it; `start` is reduced (start - ring_base < ring_len where start >= ring_base).
struct Kv8RingAppendItem {
  const unsigned short* qkv;
  unsigned char *q8, *k, *v;
  float* v_scale;
  RopeArgs ra;
  int ld, ring_base, ring_len, start;
};
struct Kv8RingAppendMultiArgs {
  Kv8RingAppendItem item[kMultiItems];
  int slab0[kMultiItems + 1];          // slab workgroups [slab0[i], slab0[i + 1]) are item[i]'s: (frame, kv head), head fastest
  int row0[kMultiItems + 1];           // rows [row0[i], row0[i + 1]) of the launch belong to item[i]
  const unsigned short *wq, *wk;
  int dim, head_dim, kv_heads, group_tokens;
  float eps;
};
static_assert(sizeof(Kv8RingAppendMultiArgs) <= 4096, "the item table travels in the kernel arguments");

// ---- the ranges launch over a two-segment key map (include/inferix_hip_kv8_magi.h): up to 8 (query range, key range) pairs of ONE
// cache.  A range's logical keys are at most two runs of consecutive slots, A = [a0, a1) (in place) and B = [b0, b1) (the scratch
// tail), either of which may be empty; the kernel walks the 64-key tiles of A, then those of B (attn_kv8_tile's kSeg form).
constexpr int kRanges = IFX_KV8_RANGES_MAX;
constexpr int kRangeStreams = IFX_KV8_RANGES_MAX_STREAMS;
static_assert(kRanges == 1 << kItemBits, "a raster word names a range in the item bits");

struct AttnKv8Range {
  int q0, q_rows, row_tiles;           // query rows [q0, q0 + q_rows) of the launch
  int a0, a1, b0, b1;                  // slots of the two runs
};
struct AttnKv8RangesArgs {
  const unsigned char* q;
  unsigned short* out;
  const unsigned char *k, *v;
  const float* v_scale;
  int ldq, ldo, group, pitch;          // group = heads / kv_heads; pitch = bytes of a cache row
  AttnKv8Range range[kRanges];         // in launch order (RangesPlan::order)
  unsigned stream[kRangeStreams];      // raster words (tile0 << 12 | kv head << 3 | range), XCD 0's list first
  int xcd_first[kXcds + 1];
  int xcd_tiles[kXcds];
};
static_assert(sizeof(AttnKv8RangesArgs) <= 4096, "the raster table travels in the kernel arguments");

// the two runs of logical keys [ks, ke) under the map (seg_split 0 = none)
inline void seg_runs(int ks, int ke, int seg_split, int seg_base, AttnKv8Range& r) {
  if (seg_split <= 0) {
    r.a0 = ks, r.a1 = ke, r.b0 = r.b1 = 0;
    return;
  }
  r.a0 = ks < seg_split ? ks : 0, r.a1 = ks < seg_split ? (ke < seg_split ? ke : seg_split) : 0;
  const int lo = ks > seg_split ? ks : seg_split;
  r.b0 = ke > seg_split ? seg_base + (lo - seg_split) : 0, r.b1 = ke > seg_split ? seg_base + (ke - seg_split) : 0;
}
// tiles of the cut walk over [ks, ke)
inline int seg_key_tiles(int ks, int ke, int seg_split) {
  AttnKv8Range r;
  seg_runs(ks, ke, seg_split, seg_split, r);
  return (r.a1 - r.a0 + kKeys - 1) / kKeys + (r.b1 - r.b0 + kKeys - 1) / kKeys;
}

struct RangesPlan {
  int n_streams, grid;
  int order[kRanges];                  // order[i] = the caller's index of launch range i: longest key range first (stable)
  int key_tiles[kRanges];              // per range, the caller's order
  int xcd_first[kXcds + 1], xcd_tiles[kXcds];
  long long xcd_cost[kXcds];
  int range[kRangeStreams], kv_head[kRangeStreams], tile0[kRangeStreams];      // per stream, in list order; range = launch position
};

// plan_multi's split with a stream = (range, kv head): `group` query heads x row tiles.  IFX_OK, IFX_EINVAL or IFX_EUNSUP.
inline int plan_ranges(const int* qr, const int* kr, int n, int heads, int kv_heads, int seg_split, RangesPlan& p) {
  if (!qr || !kr || n < 1 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || seg_split < 0) return IFX_EINVAL;
  if (n > kRanges) return IFX_EUNSUP;
  for (int i = 0; i < n; ++i)
    if (qr[2 * i] < 0 || qr[2 * i + 1] < qr[2 * i] || kr[2 * i] < 0 || kr[2 * i + 1] <= kr[2 * i]) return IFX_EINVAL;
  if ((long long)n * kv_heads > kRangeStreams || kv_heads >= (1 << kHeadBits)) return IFX_EUNSUP;
  const int group = heads / kv_heads;
  p = RangesPlan{};
  for (int i = 0; i < n; ++i) p.key_tiles[i] = seg_key_tiles(kr[2 * i], kr[2 * i + 1], seg_split);
  auto keys = [&](int i) { return p.key_tiles[i]; };
  auto tiles = [&](int i) { return (long long)group * ((qr[2 * i + 1] - qr[2 * i] + kRows - 1) / kRows); };
  for (int i = 0; i < n; ++i) {
    int j = i;
    for (; j > 0 && kr[2 * i + 1] - kr[2 * i] > kr[2 * p.order[j - 1] + 1] - kr[2 * p.order[j - 1]]; --j) p.order[j] = p.order[j - 1];
    p.order[j] = i;
  }
  // streams in order of non-increasing cost (stable over launch position, kv head), each to the XCD with the least cost so far
  int s_range[kRangeStreams], s_head[kRangeStreams], s_xcd[kRangeStreams], ns = 0;
  for (int i = 0; i < n; ++i)
    for (int h = 0; h < kv_heads && tiles(p.order[i]) > 0; ++h) {
      const long long c = tiles(p.order[i]) * keys(p.order[i]);
      int j = ns++;
      for (; j > 0 && c > tiles(p.order[s_range[j - 1]]) * keys(p.order[s_range[j - 1]]); --j) s_range[j] = s_range[j - 1], s_head[j] = s_head[j - 1];
      s_range[j] = i, s_head[j] = h;
    }
  int count[kXcds] = {};
  for (int s = 0; s < ns; ++s) {
    int x = 0;
    for (int y = 1; y < kXcds; ++y)
      if (p.xcd_cost[y] < p.xcd_cost[x]) x = y;
    s_xcd[s] = x;
    p.xcd_cost[x] += tiles(p.order[s_range[s]]) * keys(p.order[s_range[s]]);
    ++count[x];
  }
  for (int x = 0; x < kXcds; ++x) p.xcd_first[x + 1] = p.xcd_first[x] + count[x];
  // an XCD's list: longest key range first, ties in the order of assignment
  int fill[kXcds];
  for (int x = 0; x < kXcds; ++x) fill[x] = p.xcd_first[x];
  for (int s = 0; s < ns; ++s) {
    const int x = s_xcd[s];
    int j = fill[x]++;
    for (; j > p.xcd_first[x] && keys(p.order[s_range[s]]) > keys(p.order[p.range[j - 1]]); --j) p.range[j] = p.range[j - 1], p.kv_head[j] = p.kv_head[j - 1];
    p.range[j] = s_range[s], p.kv_head[j] = s_head[s];
  }
  long long most = 0;
  for (int x = 0; x < kXcds; ++x) {
    long long t = 0;
    for (int s = p.xcd_first[x]; s < p.xcd_first[x + 1]; ++s) {
      if (t >= kMaxTile0) return IFX_EUNSUP;
      p.tile0[s] = (int)t;
      t += tiles(p.order[p.range[s]]);
    }
    if (t >= kMaxTile0) return IFX_EUNSUP;
    p.xcd_tiles[x] = (int)t;
    most = most > t ? most : t;
  }
  p.n_streams = ns;
  p.grid = kXcds * (int)most;
  return IFX_OK;
}

}  // namespace kv8
}  // namespace ifx

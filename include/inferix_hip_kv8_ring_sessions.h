/* inferix_hip_kv8_ring_sessions.h — C ABI of libinferix_hip.so for several concurrent sessions over 8-bit (e4m3) RING caches
 * (inferix_hip_kv8_ring.h): the append — with the calibration of the new frames' V scales — and the grouped self-attention of up to
 * 8 samples of a ragged forward, each with a cache and a scale table of its own, in ONE launch each.
 *
 * A seventh header beside inferix_hip.h, on the terms of inferix_hip_kv8_ring.h: what is declared here is exported by the same
 * library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the symbols below: look
 * them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of inferix_hip.h, the only header
 * included here; the numeric contract of every byte is that of inferix_hip_kv8_ring.h.  The item structs carry the fields of an
 * ifx_kv8_ring_view themselves (k, v, v_scale, num_slots); kv_heads, head_dim and group_tokens are shared by a launch.
 *
 * The V scale of a frame (a group of group_tokens = G slots) and kv head, as the append below computes it from the frame's own rows:
 *   the smallest power of two s with max(amax, 2^-20) <= 448 s, amax the largest |v| over the frame's G rows x 128 channels.
 * That is exp2(ceil(log2(max(amax, 2^-20) / 448))) evaluated exactly: an amax of 7 * 2^j gives 2^(j - 6), the next bf16 above it
 * 2^(j - 5), and a frame of zeros 2^-28.
 */
#ifndef INFERIX_HIP_KV8_RING_SESSIONS_H
#define INFERIX_HIP_KV8_RING_SESSIONS_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_KV8_RING_MULTI_MAX_ITEMS 8
/* (item, head) pairs the attention launch's raster table holds in the kernel arguments: 8 items x 40 heads */
#define IFX_KV8_RING_MULTI_MAX_STREAMS 320

/* One append of a ragged batch into a ring cache: `rows` tokens of qkv [rows, >= 3 * dim] bf16, virtual positions start + r, into
 * q8_out [rows, dim] bytes (dense) and the cache k, v [num_slots, kv_heads, head_dim] bytes whose slots [0, ring_base) are fixed and
 * whose slots [ring_base, ring_base + ring_len) are a ring (ifx_rmsnorm_rope_kv8_append_ring). */
typedef struct {
  const ifx_bf16* qkv;         /* device */
  uint8_t* q8_out;             /* device */
  const ifx_rope_grid* rope;   /* host struct; read during the call.  Not NULL, flags 0; q_scale is this item's */
  uint8_t* k;                  /* device */
  uint8_t* v;                  /* device */
  float* v_scale;              /* device, [num_slots / group_tokens][kv_heads]: the rows of the groups appended to are WRITTEN */
  int32_t qkv_row_stride;      /* elements, % 8, >= 3 * dim */
  int32_t num_slots;
  int32_t ring_base;
  int32_t ring_len;
  int32_t start;
  int32_t rows;
} ifx_kv8_ring_append_item;

/* Up to IFX_KV8_RING_MULTI_MAX_ITEMS appends in ONE launch, each with the calibration of the frames it writes.  Per item and frame f
 * of its rows (rows [f G, (f + 1) G), one group of slots) and kv head: v_scale[group][head] <- the scale stated above, then the q8, K
 * and V bytes are those of ifx_rmsnorm_rope_kv8_append_ring(qkv, qkv_row_stride, q8_out, wq, wk, rope, {k, v, v_scale, num_slots,
 * kv_heads, head_dim, group_tokens}, ring_base, ring_len, start, rows, dim, eps, stream) with those scales set.  Scale rows of groups
 * not appended to and every other byte keep what they hold.  Workgroups of two kinds, none waiting for another: one per (item, frame,
 * kv head) reads the frame's V slab twice (amax, then bytes), the others are one wave per token for q and K.  `items` is a HOST array;
 * wq, wk, eps and the shape are shared.  A later launch on the same stream may read the scales through any address space.
 * IFX_EINVAL: n_items outside 1 .. 8, per item what the single call refuses with it, and start, ring_base, ring_len or rows no
 * multiple of group_tokens (a frame then lies in exactly one group).  IFX_EUNSUP: head_dim != 128, rows wider than 3072 channels. */
int ifx_rmsnorm_rope_kv8_append_ring_multi(const ifx_kv8_ring_append_item* items, int32_t n_items, const ifx_bf16* wq, const ifx_bf16* wk,
                                           int32_t kv_heads, int32_t head_dim, int32_t group_tokens, int32_t dim, float eps, void* stream);

/* One grouped self-attention of a ragged batch: `q_rows` rows of one sample attend slots [0, kv_len) of THAT sample's ring cache
 * k, v [num_slots, kv_heads, 128] bytes with the scale table v_scale [num_slots / group_tokens][kv_heads].  q8 / out as in
 * ifx_attn_fwd_kv8: row strides ldq in bytes, ldo in elements (0 = heads * 128). */
typedef struct {
  const uint8_t* q8;           /* device */
  int32_t ldq;
  int32_t ldo;
  ifx_bf16* out;               /* device */
  const uint8_t* k;            /* device */
  const uint8_t* v;            /* device */
  const float* v_scale;        /* device */
  int32_t num_slots;           /* a multiple of group_tokens */
  int32_t q_rows;
  int32_t kv_len;
} ifx_attn_kv8_grouped_item;

/* Up to IFX_KV8_RING_MULTI_MAX_ITEMS launches of ifx_attn_fwd_kv8_grouped in ONE launch: item i is
 *   ifx_attn_fwd_kv8_grouped(q8, ldq, out, ldo, NULL, {k, v, v_scale, num_slots, kv_heads, 128, group_tokens}, q_rows, heads, kv_len, stream)
 * and its output is bit-identical to that call: every item keeps the per-group tile walk and the per-tile arithmetic of its own launch,
 * only the workgroup prologue, which resolves the work item, differs.  No LSE.  `items` is a HOST array; items with q_rows == 0 are
 * checked and skipped.  The work split is ifx_attn_kv8_grouped_multi_plan's.
 * IFX_EINVAL: n_items outside 1 .. 8, and per item what ifx_attn_fwd_kv8_grouped refuses with it.  IFX_EUNSUP: a cache of 2 GiB or more;
 * n_items * heads above IFX_KV8_RING_MULTI_MAX_STREAMS or 2^20 or more row tiles on one XCD: the caller then launches the items one
 * by one. */
int ifx_attn_fwd_kv8_grouped_multi(const ifx_attn_kv8_grouped_item* items, int32_t n_items, int32_t heads, int32_t kv_heads,
                                   int32_t group_tokens, void* stream);

/* The work split of ifx_attn_fwd_kv8_grouped_multi, computed on the host with no GPU call: that of ifx_attn_kv8_multi_plan
 * (inferix_hip_kv8_sessions.h: streams, their assignment to XCDs, the raster) with a stream's cost row_tiles * key_tiles counted as the
 * grouped launch walks the keys, key_tiles = (kv_len / G) * ceil(G / 64) + ceil((kv_len % G) / 64), and the lists ordered by it. */
typedef struct {
  int32_t n_streams;                             /* (items with rows) * heads */
  int32_t grid;                                  /* 8 * max_x xcd_tiles[x] workgroups of 512 threads */
  int32_t lds_bytes;                             /* as ifx_kv8_plan.lds_bytes */
  int32_t arg_bytes;                             /* kernel-argument bytes: item structs + raster table (<= 4096) */
  int32_t order[IFX_KV8_RING_MULTI_MAX_ITEMS];   /* the caller's item indices, longest key range first (stable); [n_items] valid */
  int32_t xcd_first[9];                          /* streams [xcd_first[x], xcd_first[x + 1]) are XCD x's list, in run order */
  int32_t xcd_tiles[8];                          /* row tiles of XCD x */
  int64_t xcd_cost[8];                           /* sum of the stream costs of XCD x */
} ifx_kv8_grouped_multi_plan;

/* q_rows, kv_len: host arrays [n_items].  stream_item (the caller's item index), stream_head, stream_tile0: host arrays of `capacity`
 * entries written for the n_streams streams in list order (capacity >= n_items * heads suffices).
 * IFX_EINVAL: null pointers, n_items outside 1 .. 8, heads <= 0, group_tokens <= 0, q_rows < 0, kv_len <= 0, capacity too small.
 * IFX_EUNSUP: a set whose table does not fit, as above. */
int ifx_attn_kv8_grouped_multi_plan(const int32_t* q_rows, const int32_t* kv_len, int32_t n_items, int32_t heads, int32_t group_tokens,
                                    ifx_kv8_grouped_multi_plan* plan, int32_t* stream_item, int32_t* stream_head, int32_t* stream_tile0,
                                    int32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_RING_SESSIONS_H */

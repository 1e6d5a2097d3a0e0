/* inferix_hip_kv8_sessions.h — C ABI of libinferix_hip.so for several concurrent sessions over 8-bit (e4m3) self-attention caches:
 * the append and the self-attention of up to 8 samples of a ragged forward, each with a cache of its own, in ONE launch each.
 *
 * A fourth header beside inferix_hip.h, on the terms of inferix_hip_sessions.h and inferix_hip_kv8.h: what is declared here is
 * exported by the same library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks
 * the symbols below: look them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of
 * inferix_hip.h, the only header included here; the numeric contract of every byte is that of inferix_hip_kv8.h.  The item structs
 * carry the fields of an ifx_kv8_view themselves (k, v, v_scale, num_slots); kv_heads and head_dim are shared by a launch.
 */
#ifndef INFERIX_HIP_KV8_SESSIONS_H
#define INFERIX_HIP_KV8_SESSIONS_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_KV8_MULTI_MAX_ITEMS 8
/* (item, head) pairs the attention launch's raster table holds in the kernel arguments: 8 items x 40 heads */
#define IFX_KV8_MULTI_MAX_STREAMS 320

/* One self-attention of a ragged batch over an 8-bit cache: `q_rows` rows of one sample attend keys [kv_start, kv_len) of THAT
 * sample's cache k, v [num_slots, kv_heads, 128] bytes.  q8 / out as in ifx_attn_fwd_kv8: row strides ldq in bytes, ldo in elements
 * (0 = heads * 128). */
typedef struct {
  const uint8_t* q8;           /* device */
  int32_t ldq;
  int32_t ldo;
  ifx_bf16* out;               /* device */
  const uint8_t* k;            /* device */
  const uint8_t* v;            /* device */
  const float* v_scale;        /* device, [kv_heads] */
  int32_t num_slots;
  int32_t q_rows;
  int32_t kv_start;
  int32_t kv_len;
} ifx_attn_kv8_item;

/* Up to IFX_KV8_MULTI_MAX_ITEMS launches of ifx_attn_fwd_kv8 in ONE launch: item i is
 *   ifx_attn_fwd_kv8(q8, ldq, out, ldo, NULL, {k, v, v_scale, num_slots, kv_heads, 128}, q_rows, heads, kv_start, kv_len, stream)
 * and its output is bit-identical to that call: every item keeps the 64-key tile sequence and the per-tile arithmetic of its own
 * launch, only the workgroup prologue, which resolves the work item, differs.  No LSE.  `items` is a HOST array; items with
 * q_rows == 0 are checked and skipped.  The work split is ifx_attn_kv8_multi_plan's.
 * IFX_EINVAL: n_items outside 1 .. 8, and per item what ifx_attn_fwd_kv8 refuses with it (null pointers, q_rows < 0, heads % kv_heads,
 * keys outside [0, num_slots], strides too small or misaligned).  IFX_EUNSUP: a cache of 2 GiB or more; n_items * heads above
 * IFX_KV8_MULTI_MAX_STREAMS or 2^20 or more row tiles on one XCD (the raster table travels in the kernel arguments and does
 * not hold them): the caller then launches the items one by one. */
int ifx_attn_fwd_kv8_multi(const ifx_attn_kv8_item* items, int32_t n_items, int32_t heads, int32_t kv_heads, void* stream);

/* The work split of ifx_attn_fwd_kv8_multi, computed on the host with no GPU call.
 * A STREAM is one (item, head) pair with rows; its cost is row_tiles(item) * key_tiles(item) (256 rows and 64 keys per tile).  All row
 * tiles of a stream run on ONE XCD, so the stream's K / V are read from that XCD's L2.  Streams are taken in order of non-increasing
 * cost (ties: position in `order`, then head) and each goes to the XCD with the least cost so far (ties: the lowest), hence
 *   max_x xcd_cost[x] <= mean_x xcd_cost[x] + the largest stream cost.
 * Within an XCD streams run longest key range first (ties keep the order of assignment): the expensive tiles are not the tail.
 * Workgroup b belongs to XCD b & 7 and runs local tile b >> 3 of that XCD's list: stream s of XCD x owns the local tiles
 * [stream_tile0[s], stream_tile0[s] + row_tiles) for xcd_first[x] <= s < xcd_first[x + 1]; workgroups past xcd_tiles[x] return.
 * (b & 7 being the XCD is what ifx_attn_fwd_kv8 assumes too; only speed rests on it.) */
typedef struct {
  int32_t n_streams;                        /* (items with rows) * heads */
  int32_t grid;                             /* 8 * max_x xcd_tiles[x] workgroups of 512 threads */
  int32_t lds_bytes;                        /* as ifx_kv8_plan.lds_bytes: 3 * (64 * 128 + 128 * 64 + 32 * 16) */
  int32_t arg_bytes;                        /* kernel-argument bytes: item structs + raster table (<= 4096) */
  int32_t order[IFX_KV8_MULTI_MAX_ITEMS];   /* the caller's item indices, longest key range first (stable); [n_items] valid */
  int32_t xcd_first[9];                     /* streams [xcd_first[x], xcd_first[x + 1]) of the arrays below are XCD x's list, in run order */
  int32_t xcd_tiles[8];                     /* row tiles of XCD x */
  int64_t xcd_cost[8];                      /* sum of the stream costs of XCD x */
} ifx_kv8_multi_plan;

/* q_rows, kv_start, kv_len: host arrays [n_items].  stream_item (the caller's item index), stream_head, stream_tile0: host arrays of
 * `capacity` entries written for the n_streams streams in list order (capacity >= n_items * heads suffices).
 * IFX_EINVAL: null pointers, n_items outside 1 .. 8, heads <= 0, q_rows < 0, kv_start < 0, kv_len <= kv_start, capacity too small.
 * IFX_EUNSUP: a set whose table does not fit, as above. */
int ifx_attn_kv8_multi_plan(const int32_t* q_rows, const int32_t* kv_start, const int32_t* kv_len, int32_t n_items, int32_t heads,
                            ifx_kv8_multi_plan* plan, int32_t* stream_item, int32_t* stream_head, int32_t* stream_tile0,
                            int32_t capacity);

/* One append of a ragged batch: `rows` tokens of qkv [rows, >= 3 * dim] bf16 go through ifx_rmsnorm_rope_kv8_append into q8_out
 * [rows, dim] bytes (dense) and slots [local_start, local_start + rows) of the cache k, v [num_slots, kv_heads, head_dim] bytes. */
typedef struct {
  const ifx_bf16* qkv;         /* device */
  uint8_t* q8_out;             /* device */
  const ifx_rope_grid* rope;   /* host struct; read during the call.  Not NULL, flags 0; q_scale is this item's */
  uint8_t* k;                  /* device */
  uint8_t* v;                  /* device */
  const float* v_scale;        /* device, [kv_heads] */
  int32_t qkv_row_stride;      /* elements, % 8, >= 3 * dim */
  int32_t num_slots;
  int32_t local_start;
  int32_t rows;
} ifx_kv8_append_item;

/* Up to IFX_KV8_MULTI_MAX_ITEMS calls of ifx_rmsnorm_rope_kv8_append in ONE launch over the rows of all items (one wave per token):
 * item i's bytes (q8, K, V) are identical to ifx_rmsnorm_rope_kv8_append(qkv, qkv_row_stride, q8_out, wq, wk, rope, {k, v, v_scale,
 * num_slots, kv_heads, head_dim}, local_start, rows, dim, eps, stream).  Sessions sit at different frames: every item has its own
 * rope grid (start frame, q_scale), cache, v_scale and local_start; wq, wk, eps and the shape are shared.  `items` is a HOST array.
 * IFX_EINVAL: n_items outside 1 .. 8, and per item what the single call refuses with it.  IFX_EUNSUP: head_dim != 128, rows wider
 * than 3072 channels. */
int ifx_rmsnorm_rope_kv8_append_multi(const ifx_kv8_append_item* items, int32_t n_items, const ifx_bf16* wq, const ifx_bf16* wk,
                                      int32_t kv_heads, int32_t head_dim, int32_t dim, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_SESSIONS_H */

/* inferix_hip_kv8_ring.h — C ABI of libinferix_hip.so for the 8-bit (e4m3) self-attention cache that ROLLS: a ring placement of the
 * appended rows, so that the eviction of a rolling window moves nothing, and a V scale per GROUP of slots (a frame) instead of one
 * per cache, so that a cache that runs for an unbounded time never saturates on a scale calibrated long ago.
 *
 * A sixth header beside inferix_hip.h, on the terms of inferix_hip_kv8_split.h: what is declared here is exported by the same
 * library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the symbols below: look
 * them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of inferix_hip.h, the only header
 * included here.
 *
 * Numeric contract: every K, V and q byte and the rounding of P are those of inferix_hip_kv8.h, but for the V scale.
 *   Slots are cut into groups of group_tokens = G: group g is slots [g G, (g + 1) G).  v_scale is a device table
 *   [num_slots / G][kv_heads] of fp32, and the V bytes of group g are e4m3(clamp(v / v_scale[g][head])).  A scale may change whenever
 *   all rows of its group are rewritten with it.  The attention kernel keeps O in units of the scale of the group it is in and
 *   multiplies it by scale[g - 1] / scale[g] where the scale changes from one group to the next: exact when the scales are powers of
 *   two (the caller's calibration: exp2(ceil(log2(max(amax, 2^-20) / 448))) of the rows stored), rounded to fp32 otherwise.
 *   out = O * scale[last group] / sum, rounded to bf16 once; LSE as in inferix_hip_kv8.h.
 */
#ifndef INFERIX_HIP_KV8_RING_H
#define INFERIX_HIP_KV8_RING_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One (request, layer) of an 8-bit ring cache: k, v [num_slots, kv_heads, head_dim] bytes, contiguous. */
typedef struct {
  uint8_t* k;                  /* device */
  uint8_t* v;                  /* device */
  const float* v_scale;        /* device, [num_slots / group_tokens][kv_heads] */
  int32_t num_slots;           /* capacity in tokens, a multiple of group_tokens */
  int32_t kv_heads;
  int32_t head_dim;            /* 128 */
  int32_t group_tokens;        /* G: slots that share a V scale (the tokens of a frame) */
} ifx_kv8_ring_view;

/* What ifx_attn_fwd_kv8_grouped launches for a shape; computed on the host, no GPU call.  The fields of ifx_kv8_plan, with the key
 * tiles counted per group: a group's tiles start at the group's first slot, so its last tile is partial unless G % 64 == 0. */
typedef struct {
  int32_t row_tiles;           /* ceil(q_rows / 256) */
  int32_t key_tiles;           /* (kv_len / G) * tiles_per_group + ceil((kv_len % G) / 64): the tiles a workgroup walks */
  int32_t per_xcd;             /* as ifx_kv8_plan */
  int32_t grid;                /* 8 * per_xcd workgroups of 512 threads */
  int32_t ring;                /* K / V tile slots in LDS (3) */
  int32_t lds_bytes;           /* as ifx_kv8_plan */
  int32_t tiles_per_group;     /* ceil(G / 64) */
  int32_t groups;              /* ceil(kv_len / G): the last one may be partial */
} ifx_kv8_grouped_plan;

/* ifx_rmsnorm_rope_kv8_append (inferix_hip_kv8.h: same arguments, same bytes per row) into a cache whose slots [0, ring_base) are
 * fixed and whose slots [ring_base, ring_base + ring_len) are a ring.  Row r has the virtual position p = start + r; it goes to slot p
 * if p < ring_base, otherwise to slot ring_base + (p - ring_base) % ring_len, and its V bytes are e4m3(clamp(v / v_scale[slot / G][head])).
 * Nothing else is read or written; the caller sets the scales of the groups written before the launch (same stream).
 * IFX_EINVAL: what ifx_rmsnorm_rope_kv8_append refuses with it (but for its append range); start < 0, ring_base < 0, ring_len <= 0,
 * ring_base + ring_len > num_slots, rows > ring_len, group_tokens <= 0, num_slots % group_tokens.
 * IFX_EUNSUP: head_dim != 128, rows wider than 3072 channels. */
int ifx_rmsnorm_rope_kv8_append_ring(const ifx_bf16* qkv, int32_t qkv_row_stride, uint8_t* q8_out, const ifx_bf16* wq, const ifx_bf16* wk,
                                     const ifx_rope_grid* rope, const ifx_kv8_ring_view* view, int32_t ring_base, int32_t ring_len,
                                     int32_t start, int32_t rows, int32_t dim, float eps, void* stream);

/* ifx_attn_fwd_kv8 (inferix_hip_kv8.h: q8, ldq, out, ldo, lse as there) over slots [0, kv_len) in physical order with the scale of
 * each slot's group: softmax over that key set (key order does not matter to it).  kv_len need not be a multiple of G.
 * With equal scales in every group and G % 64 == 0 the result is bit-identical to ifx_attn_fwd_kv8 on the same bytes.
 * IFX_EINVAL: null pointers, q_rows < 0, heads % kv_heads, kv_len <= 0 or > num_slots, group_tokens <= 0, num_slots % group_tokens,
 * strides too small or misaligned.  IFX_EUNSUP: head_dim != 128, a cache of 2 GiB or more.  q_rows == 0 returns IFX_OK. */
int ifx_attn_fwd_kv8_grouped(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const ifx_kv8_ring_view* view,
                             int32_t q_rows, int32_t heads, int32_t kv_len, void* stream);

/* The launch plan of ifx_attn_fwd_kv8_grouped.  IFX_EINVAL: plan NULL, q_rows <= 0, heads <= 0, group_tokens <= 0, kv_len <= 0. */
int ifx_attn_kv8_grouped_plan(int32_t q_rows, int32_t heads, int32_t group_tokens, int32_t kv_len, ifx_kv8_grouped_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_RING_H */

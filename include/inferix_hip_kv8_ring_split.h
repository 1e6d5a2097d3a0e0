/* inferix_hip_kv8_ring_split.h — C ABI of libinferix_hip.so for the split-key form of the GROUPED self-attention over an 8-bit (e4m3)
 * ring cache: the group walk of ifx_attn_fwd_kv8_grouped (inferix_hip_kv8_ring.h) cut into chunks that run as independent workgroups
 * and are merged in the same launch by whichever chunk of a (head, row tile) finishes last, as ifx_attn_fwd_kv8_split
 * (inferix_hip_kv8_split.h) does for the flat cache.  For launches with few query rows over a long window (a 1-frame forward: 1560 rows
 * x 12 heads are 84 work items of ifx_attn_fwd_kv8_grouped on 256 CUs).
 *
 * An eighth header beside inferix_hip.h, on the terms of inferix_hip_kv8_split.h and inferix_hip_kv8_ring.h: what is declared here is
 * exported by the same library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the
 * symbols below: look them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of
 * inferix_hip.h, the only header included here; the numeric contract of every byte is that of inferix_hip_kv8_ring.h.  The fields of an
 * ifx_kv8_ring_view (k, v, v_scale, num_slots, kv_heads, group_tokens) are plain arguments; head_dim is 128.
 *
 * Numerics.  A chunk is ifx_attn_fwd_kv8_grouped's walk over its own tiles — it may begin and end inside a group — with its own lazy
 * maximum, P rounded to e4m3 and O rescaled where the V scale changes from one group to the next.  It ends in fp32 partial results: the
 * unnormalised O_c in units of s_c, the V scale of the chunk's LAST group; the lazy maximum m_c; the row sum l_c.  The merge takes them
 * IN CHUNK ORDER, whatever the order of arrival, and reads every s_c from the scale table:
 *   M = max_c m_c,  w_c = exp2(m_c - M),  out = (sum_c w_c s_c O_c) / (sum_c w_c l_c) rounded to bf16 once,
 *   LSE = (M - 7 + log2 sum_c w_c l_c) ln 2.
 * The sum is kept in units of the last chunk's scale s: the weight of chunk c is w_c (s_c / s) and the result is multiplied by
 * s / sum_c w_c l_c.  With scales that are powers of two (the ring cache's calibration) s_c / s is exact and this IS the formula above;
 * with equal scales and G % 64 == 0 a launch of n chunks is bit-identical to ifx_attn_fwd_kv8_split with n chunks on the same bytes.
 * A launch is bit-reproducible from run to run.  It is NOT bit-identical to ifx_attn_fwd_kv8_grouped when chunks > 1 (a chunk's lazy
 * maximum starts over, so P is rounded on another grid); the two agree to the rounding of P and of the merge.
 *
 * Library option (ifx_set_option / ifx_get_option of inferix_hip.h):
 *   "attn_kv8_grouped_split_min_tiles": 1 .. 65536, default 62 (env IFX_ATTN_KV8_GROUPED_SPLIT_MIN_TILES): the fewest 64-key tiles a
 *                               chunk may hold when the plan chooses the chunk count itself (num_splits = 0).  62 is the smallest chunk
 *                               at which the chosen split was measured faster than the unsplit grouped launch (1560 rows x 12 heads
 *                               over 7800 keys in 2 chunks of 63 / 62 tiles: 0.148 against 0.164 ms; at 50 tiles per chunk the two
 *                               tie; profiles/r34_attn_kv8_ring_split.md).  "attn_kv8_split_min_tiles" of the flat launch is a separate
 *                               option and is not read here.
 */
#ifndef INFERIX_HIP_KV8_RING_SPLIT_H
#define INFERIX_HIP_KV8_RING_SPLIT_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_KV8_GROUPED_SPLIT_MAX 16
/* fp32 words per query row of one chunk in the workspace, as IFX_KV8_SPLIT_ROW_WORDS: O[128], m, l and two words of padding */
#define IFX_KV8_GROUPED_SPLIT_ROW_WORDS 132

/* What ifx_attn_fwd_kv8_grouped_split launches for a shape; computed on the host, no GPU call.
 * TILES are those of the grouped walk (ifx_kv8_grouped_plan): tile t is tile t % tiles_per_group of group t / tiles_per_group and
 * starts at slot group * G + 64 * (tile in group).  Chunk c covers tiles_per_chunk[c] consecutive tiles of the walk, beginning at tile
 * first_tile[c] of group first_group[c] and ending in group last_group[c], whose scale is the unit of the chunk's partial O.
 * Raster, workspace and counters are ifx_kv8_split_plan's: GROUPS of the raster are the (head, row tile) pairs, head-major; XCD x owns
 * xcd_groups[x] of them, [x * groups / 8, (x + 1) * groups / 8); workgroup b is chunk (b >> 3) % chunks of group (b >> 3) / chunks of
 * XCD b & 7, so the chunks of a group are consecutive items of one XCD.  Workspace: [counter_bytes] one int32 per group (arrivals),
 * zeroed by the launch itself, then fp32 [chunks][heads][row_tiles][8 waves][32 * IFX_KV8_GROUPED_SPLIT_ROW_WORDS] in the lane order
 * inferix_hip_kv8_split.h describes.  Nothing the workspace held before a call is read. */
typedef struct {
  int32_t chunks;                                        /* min(num_splits, key_tiles); 1 = ifx_attn_fwd_kv8_grouped's launch, no workspace */
  int32_t row_tiles;                                     /* ceil(q_rows / 256) */
  int32_t key_tiles;                                     /* (kv_len / G) * tiles_per_group + ceil((kv_len % G) / 64) */
  int32_t tiles_per_group;                               /* ceil(G / 64) */
  int32_t grid;                                          /* 8 * ceil(groups / 8) * chunks workgroups of 512 threads */
  int32_t lds_bytes;                                     /* as ifx_kv8_plan.lds_bytes */
  int32_t counter_bytes;                                 /* groups * 4 rounded up to 256; 0 when chunks == 1 */
  int32_t key_groups;                                    /* ceil(kv_len / G) scale groups in the walk: the last one may be partial */
  int64_t workspace_bytes;                               /* counter_bytes + chunks * heads * row_tiles * 256 * 132 * 4; 0 when chunks == 1 */
  int32_t tiles_per_chunk[IFX_KV8_GROUPED_SPLIT_MAX];    /* [chunks] valid: key_tiles dealt as evenly as possible, the larger chunks first */
  int32_t first_group[IFX_KV8_GROUPED_SPLIT_MAX];        /* [chunks] valid: the scale group of the chunk's first tile */
  int32_t first_tile[IFX_KV8_GROUPED_SPLIT_MAX];         /* [chunks] valid: that tile's index inside its group */
  int32_t last_group[IFX_KV8_GROUPED_SPLIT_MAX];         /* [chunks] valid: the scale group of the chunk's last tile */
  int32_t xcd_groups[8];
} ifx_kv8_grouped_split_plan;

/* num_splits 0: the plan chooses — 1 when the unsplit launch has more than 128 (head, row tile) groups, otherwise the largest s <= 16
 * with key_tiles / s >= attn_kv8_grouped_split_min_tiles (integer division) and ceil(groups / 8) * s <= 32, at least 1: no XCD is
 * given more workgroups than it has CUs (three chunks of 84 groups are 33 on an XCD of 32 and lost to two; profiles/r31_attn_kv8_split.md).
 * IFX_EINVAL: plan NULL, q_rows <= 0, heads <= 0, group_tokens <= 0, kv_len <= 0, num_splits outside [0, 16]. */
int ifx_attn_kv8_grouped_split_plan(int32_t q_rows, int32_t heads, int32_t group_tokens, int32_t kv_len, int32_t num_splits,
                                    ifx_kv8_grouped_split_plan* plan);

/* ifx_attn_fwd_kv8_grouped (q8, ldq, out, ldo, lse, the ring view's fields, q_rows, heads, kv_len as there) with the walk cut into
 * min(num_splits, key_tiles) chunks.  `workspace`: device memory, 16-byte aligned, of at least the plan's workspace_bytes; it may be
 * NULL when the plan's chunks == 1, which launches exactly what ifx_attn_fwd_kv8_grouped launches.  Launches on one workspace must be
 * ordered (one stream).  No workgroup waits for another.  The scale table is only read.
 * IFX_EINVAL: what ifx_attn_fwd_kv8_grouped refuses with it; num_splits outside [1, 16]; with chunks > 1 a workspace that is NULL,
 * misaligned or too small.  IFX_EUNSUP: a cache of 2 GiB or more.  q_rows == 0 returns IFX_OK. */
int ifx_attn_fwd_kv8_grouped_split(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const uint8_t* k, const uint8_t* v,
                                   const float* v_scale_table, int32_t num_slots, int32_t kv_heads, int32_t group_tokens, int32_t q_rows,
                                   int32_t heads, int32_t kv_len, int32_t num_splits, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_RING_SPLIT_H */

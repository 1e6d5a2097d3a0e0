/* inferix_hip_kv8_split.h — C ABI of libinferix_hip.so for the split-key form of the self-attention over an 8-bit (e4m3) cache: the
 * key range of ONE launch is cut into chunks that run as independent workgroups, and the chunks of a (head, row tile) are merged in the
 * same launch by whichever of them finishes last.  For launches with few query rows and a long cache (a 1-frame forward: 1560 rows x
 * 12 heads are 84 work items of ifx_attn_fwd_kv8 on 256 CUs).
 *
 * A fifth header beside inferix_hip.h, on the terms of inferix_hip_kv8_sessions.h: what is declared here is exported by the same
 * library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the symbols below: look
 * them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of inferix_hip.h, the only header
 * included here; the numeric contract of every byte is that of inferix_hip_kv8.h.  The fields of an ifx_kv8_view (k, v, v_scale,
 * num_slots, kv_heads) are plain arguments; head_dim is 128.
 *
 * Numerics.  A chunk is ifx_attn_fwd_kv8's loop over its own keys (same 64-key tiles counted from kv_start, same lazy maximum, P
 * rounded to e4m3) that ends in fp32 partial results instead of a normalised row: the unnormalised O, the lazy maximum m_c and the row
 * sum l_c.  The merge takes them IN CHUNK ORDER, whatever the order of arrival:
 *   M = max_c m_c,  w_c = exp2(m_c - M),  out = (sum_c w_c O_c) v_scale / (sum_c w_c l_c) rounded to bf16 once,
 *   LSE = (M - 7 + log2 sum_c w_c l_c) ln 2.
 * A launch is therefore bit-reproducible from run to run.  It is NOT bit-identical to ifx_attn_fwd_kv8 on the same shape when
 * chunks > 1 (a chunk's lazy maximum starts over, so P is rounded on another grid); the two agree to the rounding of P and of the merge.
 *
 * Library option (ifx_set_option / ifx_get_option of inferix_hip.h):
 *   "attn_kv8_split_min_tiles": 1 .. 65536, default 73 (env IFX_ATTN_KV8_SPLIT_MIN_TILES): the fewest 64-key tiles a chunk may hold when
 *                               the plan chooses the chunk count itself (num_splits = 0).  73 is the smallest chunk at which the
 *                               chosen split was measured faster than the unsplit launch (1560 rows x 12 heads over 14040 keys in
 *                               3 chunks; profiles/r31_attn_kv8_split.md): a split launch pays about 0.07 ms for its partials and merge.
 */
#ifndef INFERIX_HIP_KV8_SPLIT_H
#define INFERIX_HIP_KV8_SPLIT_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_KV8_SPLIT_MAX 16
/* fp32 words per query row of one chunk in the workspace: O[128], m, l and two words of padding (33 16-byte pieces) */
#define IFX_KV8_SPLIT_ROW_WORDS 132

/* What ifx_attn_fwd_kv8_split launches for a shape; computed on the host, no GPU call.
 * GROUPS are the (head, row tile) pairs of ifx_attn_fwd_kv8, head-major: group = head * row_tiles + tile.  XCD x owns the groups
 * [x * groups / 8, (x + 1) * groups / 8) (integer division): xcd_groups[x] of them.  Workgroup b belongs to XCD b & 7 and runs local
 * item b >> 3 of it: chunk (b >> 3) % chunks of the XCD's group (b >> 3) / chunks; workgroups past xcd_groups[x] * chunks return.  The
 * chunks of a group are thus consecutive items of one XCD (their partials and the merge meet in one L2) and a head's K / V stay on
 * one XCD, or two where a boundary falls inside the head.  Only speed rests on b & 7 being the XCD.
 * Chunk c covers tiles_per_chunk[c] whole 64-key tiles counted from kv_start, in order; the last one ends at kv_len.
 * Workspace: [counter_bytes] one int32 per group (arrivals), zeroed by the launch itself; then the partials, fp32,
 * [chunks][heads][row_tiles][8 waves][32 * IFX_KV8_SPLIT_ROW_WORDS]: the 32 rows of a wave in the order its lanes hold them (16 pieces
 * of 64 lanes x 4 floats of O, then {m, l, 0, 0} per row), so that every store instruction writes consecutive bytes.  Nothing the
 * workspace held before a call is read. */
typedef struct {
  int32_t chunks;                                /* min(num_splits, key_tiles); 1 = the unsplit kernel of ifx_attn_fwd_kv8, no workspace */
  int32_t row_tiles;                             /* ceil(q_rows / 256) */
  int32_t key_tiles;                             /* ceil((kv_len - kv_start) / 64) */
  int32_t grid;                                  /* 8 * ceil(groups / 8) * chunks workgroups of 512 threads */
  int32_t lds_bytes;                             /* as ifx_kv8_plan.lds_bytes */
  int32_t counter_bytes;                         /* groups * 4 rounded up to 256; 0 when chunks == 1 */
  int64_t workspace_bytes;                       /* counter_bytes + chunks * heads * row_tiles * 256 * 132 * 4; 0 when chunks == 1 */
  int32_t tiles_per_chunk[IFX_KV8_SPLIT_MAX];    /* [chunks] valid: key_tiles dealt as evenly as possible, the larger chunks first */
  int32_t xcd_groups[8];
} ifx_kv8_split_plan;

/* num_splits 0: the plan chooses — 1 when the unsplit launch has more than 128 groups, otherwise the largest s <= 16 with
 * groups * s <= 256 and key_tiles / s >= attn_kv8_split_min_tiles (integer division), at least 1.
 * IFX_EINVAL: plan NULL, q_rows <= 0, heads <= 0, kv_start < 0, kv_len <= kv_start, num_splits outside [0, 16]. */
int ifx_attn_kv8_split_plan(int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, int32_t num_splits, ifx_kv8_split_plan* plan);

/* ifx_attn_fwd_kv8 (q8, ldq, out, ldo, lse, the view's fields, q_rows, heads, kv_start, kv_len as there) with the keys cut into
 * min(num_splits, key_tiles) chunks.  `workspace`: device memory, 16-byte aligned, of at least the plan's workspace_bytes; it may be
 * NULL when the plan's chunks == 1, which launches exactly what ifx_attn_fwd_kv8 launches.  Launches on one workspace must be
 * ordered (one stream).  No workgroup waits for another.
 * IFX_EINVAL: what ifx_attn_fwd_kv8 refuses with it; num_splits outside [1, 16]; with chunks > 1 a workspace that is NULL, misaligned or
 * too small.  IFX_EUNSUP: a cache of 2 GiB or more.  q_rows == 0 returns IFX_OK. */
int ifx_attn_fwd_kv8_split(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const uint8_t* k, const uint8_t* v,
                           const float* v_scale, int32_t num_slots, int32_t kv_heads, int32_t q_rows, int32_t heads, int32_t kv_start,
                           int32_t kv_len, int32_t num_splits, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_SPLIT_H */

/* inferix_hip_sessions.h — C ABI of libinferix_hip.so for serving several independent sessions from one process.
 *
 * A second header beside inferix_hip.h: what is declared here is exported by the same library but is NOT part of the table that
 * IFX_ABI_MINOR versions (inferix_hip.h stays as it is; a caller that does not serve sessions never includes this file).  A library
 * older than this header lacks the symbols below: look them up before use.  Conventions (device pointers, streams, return codes,
 * ifx_last_error) are those of inferix_hip.h.
 */
#ifndef INFERIX_HIP_SESSIONS_H
#define INFERIX_HIP_SESSIONS_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_ATTN_MULTI_MAX_ITEMS 8

/* One self-attention of a ragged batch: `q_rows` query rows of one sample attend keys [kv_start, kv_len) of THAT sample's cache.
 * q / out: [q_rows, heads, 128] bf16 with row strides ldq / ldo in elements (0 = heads * 128), as ifx_attn_fwd_paged_ld. */
typedef struct {
  const ifx_bf16* q;           /* device */
  int32_t ldq;
  ifx_bf16* out;               /* device */
  int32_t ldo;
  const ifx_kv_view* kv;       /* host struct; read during the call */
  int32_t q_rows;
  int32_t kv_start;
  int32_t kv_len;
} ifx_attn_item;

/* The self-attention launches of up to IFX_ATTN_MULTI_MAX_ITEMS samples in ONE launch: item i is
 *   ifx_attn_fwd_paged_ld(q, ldq, out, ldo, NULL, kv, q_rows, heads, kv_start, kv_len, scale, 1, NULL, 0, stream)
 * on the software-pipelined kernels, and its result is bit-identical to that call in the same loop form (every item keeps the 64-key
 * tile sequence and the per-tile arithmetic of its own unsplit launch; only the workgroup prologue, which resolves the item, differs).
 * Samples of concurrent sessions sit at different positions of their videos, so their key counts differ: query tiles are handed
 * out longest key range first.  One launch uses one loop form for all items: option attn_variant 6 or 7 names the schedule (0
 * picks between the two from the items' mean row count; 1 .. 5 are not built for this entry point: IFX_EUNSUP), the exponent
 * form is taken when scale * log2(e) == 1, and option attn_mfma picks the matrix instruction (0: from the longest item's key count).
 * `items` is a HOST array.  `heads` and `scale` are shared; every view must have the same kv_heads.  All views of a launch are of
 * one kind, contiguous or paged with pages of at least 3 rows.  Under attn_variant 0 an item of fewer than 1024 rows or at most 1024
 * keys is a four-wave-kernel launch when made alone; a launch with such an item is refused (IFX_EUNSUP) and the caller launches the
 * items one by one.  IFX_EUNSUP also: a two-segment view (seg_split > 0), pages of one or
 * two rows, views of both kinds.  IFX_EINVAL: n_items outside 1 .. 8, differing kv_heads, what ifx_attn_fwd_paged_ld refuses. */
int ifx_attn_fwd_multi(const ifx_attn_item* items, int32_t n_items, int32_t heads, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_SESSIONS_H */

/* inferix_hip_kv8_magi.h — C ABI of libinferix_hip.so for MAGI's self-attention over an 8-bit (e4m3) cache: the head-prep kernel that
 * writes e4m3 q / K / V behind MAGI's per-head LayerNorm and partial rotary, and ONE attention launch for all (query range, key
 * range) pairs of a forward over a cache whose key map has two segments (rows in place + the unstored rows of this forward in a
 * scratch tail).
 *
 * A ninth header beside inferix_hip.h, on the terms of inferix_hip_kv8_sessions.h: what is declared here is exported by the same
 * library but is NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the symbols below: look
 * them up before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of inferix_hip.h, the only header
 * included here; the numeric contract of every byte (K, q, V, P, the row sum, the one rounding of out) is that of inferix_hip_kv8.h.
 * The cache's fields are plain arguments; head_dim is 128.
 */
#ifndef INFERIX_HIP_KV8_MAGI_H
#define INFERIX_HIP_KV8_MAGI_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (query range, key range) pairs of one launch */
#define IFX_KV8_RANGES_MAX 8
/* (range, kv head) pairs the raster table holds in the kernel arguments: 8 ranges x 16 kv heads */
#define IFX_KV8_RANGES_MAX_STREAMS 128

/* ifx_magi_head_prep (inferix_hip.h) layout 0 with 8-bit outputs: in = [rows, q_heads q | q_heads qx | kv_heads k | kv_heads v] x 128.
 * Per token the same fp32 LayerNorm (layernorm_1p), the same partial rotary (rope_half) and the same destination rule
 *   dest(r) = r < split ? row0 + r : row1 + (r - split)
 * as there; then
 *   q  : e4m3(clamp(rot_q * q_scale))             -> q8_out[r * ld_q8 + h * 128]                  (bytes)
 *   k  : e4m3(clamp(rot_k))                       -> k_out[dest(r) * ld_kv + h * kv_head_stride]  (bytes)
 *   v  : e4m3(clamp(v / v_scale[h]))              -> v_out[dest(r) * ld_kv + h * kv_head_stride]  (IEEE division in fp32)
 *   qx : bf16, bit-identical to ifx_magi_head_prep's -> qx_out[r * ld_qx + h * 128]
 * clamp is to [-448, 448]; the rounding is v_cvt_pk_fp8_f32's (nearest even): the byte rule of inferix_hip_kv8.h.  The values that
 * are rounded to e4m3 are the fp32 values ifx_magi_head_prep rounds to bf16 (q, k) or copies (v): there is no bf16 step in between.
 * Strides of the byte outputs are in BYTES (% 8); ld_qx in elements (% 8).
 * IFX_EINVAL: what ifx_magi_head_prep refuses for layout 0, and v_scale NULL.  IFX_EUNSUP: q_group != 0 (the all-to-all send order is
 * for the bf16 path: context parallelism moves bf16 K / V), head_dim != 128. */
typedef struct {
  const ifx_bf16* in;
  int32_t ld_in, rows, q_heads, kv_heads, head_dim;
  const float* rope;                          /* [rows, 2 * rope_half] fp32 = (sin | cos) */
  const float *qn_w, *qn_b, *kn_w, *kn_b;     /* fp32 [128] */
  const ifx_bf16 *xn_w, *xn_b;                /* bf16 [128] */
  float eps;
  int32_t layernorm_1p;
  uint8_t* q8_out;
  int32_t ld_q8;
  ifx_bf16* qx_out;
  int32_t ld_qx;
  uint8_t* k_out;
  uint8_t* v_out;
  int32_t ld_kv, kv_head_stride;
  int32_t row0, split, row1;
  float q_scale;                              /* 0 = 1 */
  int32_t rope_half;                          /* 0 = 64 */
  const float* v_scale;                       /* device, [kv_heads]; read by the kernel */
  int32_t q_group;                            /* must be 0 */
} ifx_magi_head_prep_kv8_desc;
int ifx_magi_head_prep_kv8(const ifx_magi_head_prep_kv8_desc* desc, void* stream);

/* n_ranges (1 .. 8) attentions over ONE 8-bit cache k, v [num_slots, kv_heads, 128] bytes in one launch: for range i the query rows
 * [q_ranges[2 i], q_ranges[2 i + 1]) of q8 attend the LOGICAL keys [k_ranges[2 i], k_ranges[2 i + 1]), as ifx_attn_fwd_ranges' do.
 * q8 [q_rows, heads, 128] bytes with row stride ldq (bytes, 0 = heads * 128, % 16); out bf16 with row stride ldo (elements, 0 = heads *
 * 128, % 8); rows outside every query range are not written.  Grouped-query heads: head h reads kv head h / (heads / kv_heads).  No LSE.
 *
 * Key map: logical key j lives in slot j for j < seg_split and in slot seg_base + (j - seg_split) otherwise (ifx_kv_view's
 * seg_split / seg_split + seg_delta); seg_split == 0 means no map (slot j).  A range's keys are therefore at most two runs of
 * consecutive slots, and the walk along the keys is CUT where the first run ends: 64-key tiles counted from the range's first key up
 * to seg_split — the last of them masked by index past seg_split (P = 0 exactly) and its K / V rows past the run read as zeros
 * through the descriptor bound, which is the RUN's end — then 64-key tiles counted from seg_base.  Every tile is consecutive slots
 * under one wave-uniform base.  A range that lies in one run, or whose first run is a whole number of tiles, is bit-identical to
 * ifx_attn_fwd_kv8 over a contiguous copy of its keys; otherwise the tiles are cut differently and the two agree to the rounding of P.
 *
 * IFX_EINVAL: null pointers, n_ranges < 1, heads % kv_heads, a query range outside [0, q_rows] or reversed, an empty or negative key
 * range, seg_split < 0, seg_base < seg_split, a key that maps outside [0, num_slots), strides too small or misaligned.
 * IFX_EUNSUP: n_ranges > 8, more than IFX_KV8_RANGES_MAX_STREAMS (range, kv head) pairs, 2^20 or more row tiles on one XCD: the caller
 * then launches range by range.  IFX_EUNSUP also: a cache of 2 GiB or more (byte offsets are 32-bit), for which there is no such
 * way out.  Ranges without query rows are checked and skipped. */
int ifx_attn_fwd_kv8_ranges(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, const uint8_t* k, const uint8_t* v,
                            const float* v_scale, int32_t num_slots, int32_t kv_heads, int32_t seg_split, int32_t seg_base, int32_t q_rows,
                            int32_t heads, int32_t n_ranges, const int32_t* q_ranges, const int32_t* k_ranges, void* stream);

/* The work split of ifx_attn_fwd_kv8_ranges, computed on the host with no GPU call.
 * A work unit is a (range, head, 256-row tile): a row tile never holds rows of two ranges.  A STREAM is one (range, kv head) pair with
 * query rows: all heads / kv_heads query heads of the kv head and all their row tiles, head-major — stream_tiles = (heads / kv_heads) *
 * row_tiles(range) units that read the same K / V bytes.  Its cost is stream_tiles * key_tiles(range), key_tiles counted along the cut
 * walk above.  A stream runs on ONE XCD.  Streams are taken in order of non-increasing cost (ties: position in `order`, then kv head)
 * and each goes to the XCD with the least cost so far (ties: the lowest), hence
 *   max_x xcd_cost[x] <= mean_x xcd_cost[x] + the largest stream cost.
 * Within an XCD streams run longest key range first.  Workgroup b belongs to XCD b & 7 and runs local tile b >> 3 of that XCD's list:
 * stream s of XCD x owns the local tiles [stream_tile0[s], stream_tile0[s] + stream_tiles) for xcd_first[x] <= s < xcd_first[x + 1];
 * local tile stream_tile0[s] + g * row_tiles + t is row tile t of query head kv_head * (heads / kv_heads) + g.  Workgroups past
 * xcd_tiles[x] return.  The table travels in the kernel arguments.  Only speed rests on b & 7 being the XCD. */
typedef struct {
  int32_t n_streams;                        /* (ranges with rows) * kv_heads */
  int32_t grid;                             /* 8 * max_x xcd_tiles[x] workgroups of 512 threads */
  int32_t lds_bytes;                        /* as ifx_kv8_plan.lds_bytes */
  int32_t arg_bytes;                        /* kernel-argument bytes: range structs + raster table (<= 4096) */
  int32_t order[IFX_KV8_RANGES_MAX];        /* the caller's range indices, longest key range first (stable); [n_ranges] valid */
  int32_t key_tiles[IFX_KV8_RANGES_MAX];    /* per range in the CALLER's order: tiles of the cut walk */
  int32_t xcd_first[9];
  int32_t xcd_tiles[8];
  int64_t xcd_cost[8];
} ifx_kv8_ranges_plan;

/* q_ranges, k_ranges: host arrays [2 * n_ranges].  stream_range (the caller's range index), stream_kv_head, stream_tile0: host arrays
 * of `capacity` entries written for the n_streams streams in list order (capacity >= n_ranges * kv_heads suffices).
 * IFX_EINVAL: null pointers, n_ranges < 1, heads % kv_heads, reversed or negative query ranges, empty or negative key ranges,
 * seg_split < 0, capacity too small.  IFX_EUNSUP: n_ranges > 8 or a set whose table does not fit, as above. */
int ifx_attn_kv8_ranges_plan(const int32_t* q_ranges, const int32_t* k_ranges, int32_t n_ranges, int32_t heads, int32_t kv_heads,
                             int32_t seg_split, ifx_kv8_ranges_plan* plan, int32_t* stream_range, int32_t* stream_kv_head,
                             int32_t* stream_tile0, int32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_MAGI_H */

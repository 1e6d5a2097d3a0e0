/* inferix_hip_kv8.h — C ABI of libinferix_hip.so for a self-attention KV cache held in 8 bits (OCP e4m3) and the self-attention
 * kernel that reads it on the 8-bit matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4, unit scales).
 *
 * A further header beside inferix_hip.h, as inferix_hip_sessions.h is: what is declared here is exported by the same library but is
 * NOT part of the table that IFX_ABI_MINOR versions.  A library older than this header lacks the symbols below: look them up
 * before use.  Conventions (device pointers, streams, return codes, ifx_last_error) are those of inferix_hip.h.
 *
 * Numeric contract.  Every 8-bit value is e4m3 (v_cvt_pk_fp8_f32: round to nearest even) of a value clamped to [-448, 448] first.
 *   K : e4m3 of the normalised, rotated key (no scale: RMSNorm bounds it, RoPE is a rotation).
 *   q : e4m3 of rope(norm(q)) * q_scale; with q_scale = softmax_scale * log2(e) the scores q.k are exponents of 2.
 *   V : e4m3 of v / v_scale[kv_head]; one fp32 scale per KV head and view, the same for every row the cache holds (the caller may
 *       change it only together with an append that rewrites every row attended afterwards, i.e. one that starts at slot 0).
 *   P : exp2(s - m + 7) rounded to e4m3; m is a lazy row maximum that lags the true one by at most 1.75 (2^8.75 < 448).
 *   The row sum is accumulated in fp32 from the unrounded P; out = acc * v_scale / sum, rounded to bf16 once; LSE is natural log, fp32.
 *   Accuracy of the LSE: its error grows with the magnitude of the scores, about 7e-6 of the largest |q.k| (in log2 units) of the
 *   row — 9e-4 measured at scores of 65, 2.2e-3 at 190 — because the 8-bit matrix instruction's accumulation of q.k is coarser than an
 *   fp32 FMA chain.  The output is not affected beyond the e4m3 rounding of P.
 */
#ifndef INFERIX_HIP_KV8_H
#define INFERIX_HIP_KV8_H

#include "inferix_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One (request, layer) of an 8-bit cache: k, v [num_slots, kv_heads, head_dim] bytes, contiguous; logical token t lives in slot t. */
typedef struct {
  uint8_t* k;                  /* device */
  uint8_t* v;                  /* device */
  const float* v_scale;        /* device, [kv_heads] */
  int32_t num_slots;           /* capacity in tokens */
  int32_t kv_heads;
  int32_t head_dim;            /* 128 */
} ifx_kv8_view;

/* What ifx_attn_fwd_kv8 launches for a shape; computed on the host, no GPU call. */
typedef struct {
  int32_t row_tiles;           /* ceil(q_rows / 256): query rows per workgroup are 256, 32 per wave */
  int32_t key_tiles;           /* ceil((kv_len - kv_start) / 64) */
  int32_t per_xcd;             /* work items (row tile, head) each of the 8 XCDs owns: ceil(row_tiles * heads / 8); workgroup b
                                  runs item (b & 7) * per_xcd + (b >> 3), head-major, so one head's K / V stay in one XCD's L2 */
  int32_t grid;                /* 8 * per_xcd workgroups of 512 threads */
  int32_t ring;                /* K / V tile slots in LDS (3) */
  int32_t lds_bytes;           /* ring * (64 * 128 + 128 * 64 + 32 * 16): a K tile and a transposed, padded V tile per slot */
} ifx_kv8_plan;

/* The 8-bit twin of ifx_rmsnorm_rope_kv_append (same rounding points up to the rotation: y = bf16(x * rsqrt(mean(x^2) + eps));
 * y = bf16(y * w); rotation in fp64 -> fp32), then
 *   q8_out[r, :]              = e4m3(clamp(rot_q * q_scale))        (q_scale of the rope grid; 0 = 1), [rows, dim] bytes, dense
 *   view.k[local_start + r]   = e4m3(clamp(rot_k))
 *   view.v[local_start + r]   = e4m3(clamp(v / v_scale[head]))      (IEEE division in fp32)
 * `rope` must not be NULL; its flags must be 0 (the V rows are always taken from qkv).  qkv_row_stride (elements, % 8) >= 3 * dim.
 * IFX_EINVAL: null pointers, dim != kv_heads * head_dim, dim % 8, the append range outside [0, num_slots], a bad rope grid, flags != 0.
 * IFX_EUNSUP: head_dim != 128, rows wider than 3072 channels. */
int ifx_rmsnorm_rope_kv8_append(const ifx_bf16* qkv, int32_t qkv_row_stride, uint8_t* q8_out, const ifx_bf16* wq, const ifx_bf16* wk,
                                const ifx_rope_grid* rope, const ifx_kv8_view* view, int32_t local_start, int32_t rows, int32_t dim,
                                float eps, void* stream);

/* out[r, h, :] = softmax_j(q8[r, h, :] . K[j, h / (heads / kv_heads), :] * ln 2) . V[j, ...] * v_scale,  j in [kv_start, kv_len):
 * the scores are exponents of 2 (see q above).  q8: [q_rows, heads, 128] bytes with row stride ldq (bytes, 0 = heads * 128, % 16);
 * out: bf16 with row stride ldo (elements, 0 = heads * 128, % 8); lse: optional [heads, q_rows] fp32, natural log.  One unsplit launch.
 * IFX_EINVAL: null pointers, q_rows < 0, heads % kv_heads, kv_start < 0, kv_len <= kv_start or > num_slots, strides too small or
 * misaligned.  IFX_EUNSUP: head_dim != 128, a cache of 2 GiB or more (byte offsets are 32-bit).  q_rows == 0 returns IFX_OK. */
int ifx_attn_fwd_kv8(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const ifx_kv8_view* view, int32_t q_rows,
                     int32_t heads, int32_t kv_start, int32_t kv_len, void* stream);

/* The launch plan of ifx_attn_fwd_kv8 for a shape.  IFX_EINVAL: plan NULL, q_rows <= 0, heads <= 0, kv_start < 0, kv_len <= kv_start. */
int ifx_attn_kv8_plan(int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, ifx_kv8_plan* plan);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_KV8_H */

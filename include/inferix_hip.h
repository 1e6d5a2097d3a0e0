/*
 * inferix_hip.h — C-ABI of libinferix_hip.so: the MI355X (gfx950) kernels of the
 * semi-autoregressive block-diffusion denoising step (causal Wan DiT) behind
 * Inferix's generator / attention / KV-cache interfaces.
 *
 * The reference (alibaba-damo-academy/Inferix) has no FFI layer: its hot path is
 * Python calling un-vendored CUDA libraries.  Each entry point below names the
 * reference Python call site(s) it replaces (paths relative to the reference
 * root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions (all entry points):
 *   - plain C: device pointers + sizes, no torch types; caller owns every buffer
 *     (PyTorch caching allocator or the KV-cache manager); no hidden allocation.
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); nothing
 *     synchronises.
 *   - returns 0 on success, a negative IFX_E* code otherwise; never throws.
 *     ifx_last_error() returns a thread-local human-readable message.
 *   - bf16 = IEEE bfloat16 stored as uint16_t; activations are token-major
 *     [rows, channels] with the channel dimension contiguous.
 *   - rounding points follow the reference's bf16 module boundaries (documented
 *     per function) so results match its PyTorch path to bf16 rounding noise.
 */
#ifndef INFERIX_HIP_H
#define INFERIX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IFX_OK 0
#define IFX_EINVAL (-1)   /* bad argument (null pointer, unsupported shape) */
#define IFX_ELAUNCH (-2)  /* HIP launch error */
#define IFX_EUNSUP (-3)   /* configuration not built into this library */

typedef uint16_t ifx_bf16;

/* library identity ------------------------------------------------------- */
/* The MINOR number is the ABI generation: it changes whenever an argument struct gains a field or an entry point changes its
 * signature (0.2: ifx_kv_view.seg_split / seg_delta, ifx_rope_grid.q_scale; 0.3: ifx_magi_head_prep_desc.rope_half, gemm_small_split; 0.4: ifx_gemm_q8_quant_out, ifx_layernorm_quant_static; 0.6: ifx_get_option, ifx_device_error, bounded device waits; 0.7: ifx_conv3d_desc.in_planar, IFX_NORM_OUT_PLANAR, conv_variant, attn_debug_counters).  Callers built against another minor
 * must not call in: zero-initialise every struct (new fields default to 0 = off) and compare IFX_ABI_MINOR with
 * (ifx_version() >> 8) & 255 at load time, as inferix_amd/_hip.py does. */
#define IFX_ABI_MINOR 7
int ifx_version(void);                 /* (major<<16)|(minor<<8)|patch */
const char* ifx_last_error(void);      /* thread-local, never NULL */
const char* ifx_arch(void);            /* "gfx950" */
/* Kernel-selection override for benchmarking and tests (default 0 = choose by shape):
 *   "gemm_variant": 1 register-staged 128x128; LDS-DMA tiles 2 = 256x128x64, 3 = 128x128x64 (two workgroups per CU),
 *                   4 = 64x64, 5 = 256x256x64, 6 = 128x64, 7 = 256x128x32 (two per CU), 8 = 128x128x32 (eight waves),
 *                   9 / 10 = warp-specialised 256x128 / 128x128, 11 = 256x256x32 four stages,
 *                   12 / 13 / 14 = 64x64 (four K-groups), 64x64 (two), 128x128 (two): split-K between the wave groups of one
 *                   workgroup, what 0 = auto picks for launches of at most one workgroup per CU; K / 64 must divide by the groups;
 *                   15 = 128x64 two stages (three per CU), 16 / 17 = 64x128 two / three stages,
 *                   18 = four-wave 256x256 on the LDS-DMA ring (experiment), 19 = four-wave 256x256x64 register-staged software
 *                   pipeline (ifx_gemm_w4.hip), 20 = auto including its split-K form when a workspace is given,
 *                   21 = 256x192x64 (what 0 = auto picks where 192-wide columns fill the rounds better: the QKV projection),
 *                   22 / 23 / 24 = the persistent ping-pong tiles of ifx_gemm_pp.hip: 256 / 192 / 128 tokens x 256 channels (what 0 =
 *                   auto picks for launches of at least 2048 rows); 22 and 23 split K over two workgroups per tile where N <= 2048 and
 *                   K >= 4096 when the caller gives a workspace (ifx_gemm_bf16_ws), 25 = 22 without that split,
 *                   26 = stream-K on the 128-token ping-pong tile (needs the ifx_gemm_workspace_bytes workspace; an experiment that
 *                   lost to the tiles above at every size tried, kept for the lab: profiles/r3_gemm_pp.md),
 *                   27 / 28 / 29 = the 128-token ping-pong tile with K split over 2 / 4 / 8 workgroups per tile (each part >= 1 dumps
 *                   its fp32 tile image and raises its own flag, part 0 adds them in part order; needs the ifx_gemm_workspace_bytes
 *                   workspace and K / 64 divisible by the parts).  Under gemm_small_split 0 = auto takes the 4-way form for long-K
 *                   launches whose 128 x 256 tiles x 4 make one round of 129 .. 256 work items (a 4-way rank's FFN down-projection).
 *                   ifx_gemm_q8 reads the same option: 1 / 2 = register-staged 128x128 / 64-byte-row LDS-DMA tiles, 3 = the LDS-DMA
 *                   tiles, never the ping-pong tile, 22 / 23 / 24 = the ping-pong tile with 256 / 192 / 128 tokens (FP8 and INT8)
 *   "gemm_small_split": 1 lets the auto choice split K between the wave groups of one workgroup for launches of at most one workgroup
 *                   per CU (a sequence-parallel rank's 585 .. 2340 rows).  PER HOST THREAD (set, read and applied on the calling
 *                   thread only: launches another thread enqueues meanwhile keep their own value).  Off by default: those tiles sum K in a different order and
 *                   which launches get them depends on the row count, while the default auto choice keeps a row's bits independent
 *                   of the number of rows in the launch (its only K split, two workgroups per tile for N <= 2048 and K >= 4096
 *                   through ifx_gemm_bf16_ws, is a function of N and K).
 *   "attn_variant": 1 four-wave kernel, 2 eight-wave ping-pong schedule, 3 twelve-wave three-phase schedule,
 *                   4 free-running schedule, 5 software-pipelined schedule, 6 software-pipelined in four-wave workgroups, two per CU,
 *                   7 software-pipelined and unrolled four times over constant LDS slots (what 0 = auto picks for large launches).
 *                   The one place that lists the schedules 2 .. 7 (wave groups, loop form, tile height, LDS) and holds the automatic
 *                   choice is the table `kAttnSchedules` / `attn_pick_variant` in inferix_amd/csrc/ifx_attn.h.
 * Results are identical across variants up to fp32 summation order.  Returns IFX_EINVAL for unknown keys. */
/*   "gemm_pp_variant":  0 = auto: the unsplit bf16 128-token ping-pong tile (what gemm_variant 24, or 0 on shapes like the 1536 x 1536
 *                   projections, runs) in its twelve-wave form, four LDS-DMA loader waves beside the eight compute waves (round 8); 1 = the
 *                   eight-wave form it replaced (A/B runs and tests; the same bits).  Environment fallback IFX_GEMM_PP_VARIANT. */
/*   "attn_mfma":        matrix instruction of the attn_variant 7 loop.  0 = auto: v_mfma_f32_16x16x32_bf16 for the launch classes where it
 *                   was measured faster (unsplit launches with prescaled q from 14040 keys on, whatever the view: `attn_pick_mfma16` in
 *                   inferix_amd/csrc/ifx_attn.h), v_mfma_f32_32x32x16_bf16
 *                   otherwise; 1 = 32x32x16 everywhere (the form before round 22: A/B runs and tests); 2 = 16x16x32 for every launch of
 *                   schedule 7.  Other schedules have the 32x32x16 form only.  The two forms agree to rounding, not to the bit (key
 *                   order inside a k-step, row-sum order).  Environment fallback IFX_ATTN_MFMA. */
/*   "conv_variant":     0 = auto (round 6: the persistent ping-pong kernel for 3x3 spatial kernels with cout % 96 == 0), 1 = the lock-step
 *                       kernel of round 1 everywhere (A/B: tools/bench_conv.py; the two produce identical bits).
 *   "attn_debug_counters": tests only — 1 allocates and zeroes a device word that the ping-pong attention kernels increment once per
 *                       (wave, key tile) that takes the rescale branch of the lazy row maximum; read it with
 *                       ifx_get_option("attn_rescale_count") (synchronises the device); 0 turns the counting off. */
int ifx_set_option(const char* key, int32_t value);
/* The value an option has NOW in the library (set through ifx_set_option by anyone in the process, or its environment default):
 * what a scoped override has to put back (a Python-side mirror misses options set through another binding).
 * Further keys of both calls:
 *   "spin_timeout_ms": budget of every DEVICE-side wait (the split-K / stream-K hand-off of ifx_gemm_bf16_ws / ifx_gemm_q8_ws), 1 ..
 *                      600000, default 2000 (env IFX_SPIN_TIMEOUT_MS).  A wait that runs out raises the device error word, the launch
 *                      completes with invalid results instead of hanging the GPU.
 *   "spin_fault":      tests only — 1 keeps the producers' flags down so that every such wait runs into its budget. */
int ifx_get_option(const char* key, int32_t* value);
/* Device error word: 0, or (kind << 24) | detail of the first wait a kernel gave up since the word was last cleared (kind 1 = split-K /
 * stream-K consumer, detail = flag index).  Pinned host memory: reading it needs no device synchronisation, but a launch only shows up
 * here once it has run — check after the stream has been synchronised.  `clear` != 0 resets the word.  ifx_last_error() reports (and
 * clears) a raised word ahead of the thread's last host-side message. */
int32_t ifx_device_error(int32_t clear);

/* ------------------------------------------------------------------------
 * Paged KV cache view (one request, one layer).
 * Replaces the tensors handed around by inferix/kvcache_manager/kvcache_manager.py:145-220
 * (`get` / `set`) and the slice arithmetic of
 * inferix/models/self_forcing/causal_model.py:277-304.
 *
 * Physical layout is the reference manager's own: K and V each
 * [num_slots][kv_heads][head_dim] bf16, token-major (manager tensor
 * (2, num_blocks, block_size, kv_heads, head_dim), kvcache_manager.py:222-244).
 * Logical token t lives in physical slot
 *     page_table ? page_table[t / page_size] * page_size + t % page_size : t     (or the two-segment map below)
 * so sink+rolling eviction (causal_model.py:282-300) is a page-table rotation
 * instead of a data move whenever the evicted span is page-aligned.
 * ---------------------------------------------------------------------- */
typedef struct {
  ifx_bf16* k;                 /* device */
  ifx_bf16* v;                 /* device */
  const int32_t* page_table;   /* device, may be NULL (identity) */
  int32_t page_size;           /* tokens per page (ignored when page_table == NULL) */
  int32_t num_slots;           /* capacity in tokens */
  int32_t kv_heads;
  int32_t head_dim;            /* 128 */
  /* Two-segment map for readers (the attention entry points), used when page_table == NULL and seg_split > 0: logical token
   * t < seg_split lives in slot t, t >= seg_split in slot t + seg_delta.  MAGI's cache rule leaves the rows of a forward that the
   * rule does not store outside the cache proper (inferix/kvcache_manager/model/magi_kv_cache_manager.py:76-187): here they sit in
   * a scratch tail of the same allocation and this map splices them behind the prefix without a per-token table.  0 = off.
   * ifx_rmsnorm_rope_kv_push honours the map for its stores; the other writers by logical token (ifx_rmsnorm_rope_kv_append,
   * ifx_kv_roll, ifx_kv_scatter_shards) return IFX_EINVAL for a view with seg_split > 0 and no page table. */
  int32_t seg_split;
  int32_t seg_delta;
} ifx_kv_view;

/* ------------------------------------------------------------------------
 * Block-causal flash-attention forward over the cached prefix, KV read in place.
 *   out[r,h,:] = softmax_j(q[r,h,:]·K[j,h,:] * scale) · V[j,h,:],  j in [kv_start, kv_len)
 * (logical cache tokens; kv_start > 0 is the split-KV / sequence-parallel case whose partial results
 * are combined with ifx_lse_merge)
 * No mask: block causality is realised by what is in the cache
 * (causal_model.py:307-315).  Replaces `attention()` / `flash_attention()`
 * (inferix/models/attention/flash_attention.py:42-200) and the registry backends'
 * (out, lse) contract (inferix/models/attention/backends.py:36-76).
 *   q, out : [q_rows, heads, 128] bf16 (row stride = heads*128); heads may be a multiple of kv->kv_heads
 *            (grouped-query attention, MAGI: query head h reads kv head h / (heads/kv_heads),
 *            inferix/models/magi/dit/dit_module.py:975-1018)
 *   lse    : optional [heads, q_rows] fp32 (natural log), NULL to skip
 *   scale  : softmax scale (1/sqrt(128) when <= 0)
 * bf16 in, fp32 softmax/accumulate, P rounded to bf16 for the PV product, bf16 out.
 * ---------------------------------------------------------------------- */
int ifx_attn_fwd_paged(const ifx_bf16* q, ifx_bf16* out, float* lse, const ifx_kv_view* kv,
                       int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, float scale,
                       void* stream);

/* Split-KV form of ifx_attn_fwd_paged for launches with few query rows (the sequence-parallel shards of
 * causal_model.py:939-942: N/P = 585 rows at P = 8, i.e. 36 (tile, head) pairs for 256 CUs).  The key range is cut
 * into `num_splits` chunks that run as independent workgroups; fp32 partial results go to `workspace` and are
 * combined with the ifx_lse_merge algebra (distributed.py:30-48) before the single bf16 rounding.  Result: as
 * ifx_attn_fwd_paged.  ifx_attn_split_plan returns the chunk count that fills the chip for a shape (1 = do not
 * split) and the workspace size that count needs; no allocation happens inside the library. */
int32_t ifx_attn_split_plan(int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len,
                            int64_t* workspace_bytes);
int ifx_attn_fwd_paged_split(const ifx_bf16* q, ifx_bf16* out, float* lse, const ifx_kv_view* kv,
                             int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, float scale,
                             int32_t num_splits, void* workspace, int64_t workspace_bytes, void* stream);

/* ifx_attn_fwd_paged with explicit row strides of q and out (elements, >= heads * 128): the query rows may be a column block of
 * a wider matrix and the result may be written straight into a column block of the next GEMM's input — MAGI concatenates the
 * self-attention and cross-attention outputs in front of linear_proj (inferix/models/magi/dit/dit_module.py:1281-1295); with the
 * two attention launches writing columns [0, Q) and [Q, 2Q) of one [rows, 2Q] buffer the concatenation never exists as a copy.
 * num_splits / workspace as ifx_attn_fwd_paged_split (1 / NULL = no split). */
int ifx_attn_fwd_paged_ld(const ifx_bf16* q, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const ifx_kv_view* kv,
                          int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, float scale, int32_t num_splits,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* Attention over keys [0, kv_len) in which the LAST key stands for `last_key_multiplicity` identical (key, value) rows:
 *   out = softmax over the kv_len - 1 + multiplicity implied keys — computed by adding ln(multiplicity) to the last key's score.
 * Cross-attention of the block (inferix/models/wan_base/model.py:66-100) runs over text_len = 512 context rows of which all but
 * the prompt's own tokens are the zero-padding (causal_model.py:948-953): those rows are identical after `text_embedding`, so are
 * their K and V rows in every layer, and 512 keys become n_prompt + 1 — one 64-key tile instead of eight.  Exact algebra; the
 * implied keys' probabilities are rounded to bf16 once (as one product) instead of `multiplicity` times.  kv_len <= 1024. */
int ifx_attn_fwd_dedup(const ifx_bf16* q, ifx_bf16* out, const ifx_kv_view* kv, int32_t q_rows, int32_t heads, int32_t kv_len,
                       int32_t last_key_multiplicity, float scale, void* stream);

/* Several (query range, key range) pairs of one cache in ONE launch — MAGI's core_attention (inferix/models/magi/dit/dit_module.py:
 * 972-1015): per denoising range i, queries [q_ranges[i][0], q_ranges[i][1]) attend keys [k_ranges[i][0], k_ranges[i][1]), no mask
 * inside a range.  One rank of cp = 8 has 3 query heads: a single range is 144 workgroups for 256 CUs, four ranges together fill
 * the chip without splitting keys.  q_ranges / k_ranges are HOST arrays [n_ranges][2]; 1 <= n_ranges <= 8; ranges are tiled
 * separately (a query tile never straddles two ranges) and scheduled longest key range first.  Strides as ifx_attn_fwd_paged_ld
 * (0 = dense). */
int ifx_attn_fwd_ranges(const ifx_bf16* q, int32_t ldq, ifx_bf16* out, int32_t ldo, const ifx_kv_view* kv, int32_t q_rows,
                        int32_t heads, int32_t n_ranges, const int32_t* q_ranges, const int32_t* k_ranges, float scale,
                        void* stream);

/* The same split-KV algebra in separate launches that share one workspace: under sequence parallelism the cached
 * prefix is attended while the collective that delivers the new block's keys is still in flight, then the new keys,
 * then ONE merge.  ifx_attn_fwd_partial writes the fp32 partials of up to `num_splits` key chunks of
 * [kv_start, kv_len) into slots [slot_base, slot_base + *slots_used) of a workspace laid out for `slot_cap` slots
 * (slot_cap * q_rows * heads * 129 floats); ifx_attn_merge_partials combines the first `slots_used` slots into
 * out (bf16, one rounding) and the optional lse. */
int ifx_attn_fwd_partial(const ifx_bf16* q, const ifx_kv_view* kv, int32_t q_rows, int32_t heads, int32_t kv_start,
                         int32_t kv_len, float scale, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                         int32_t slot_base, int32_t slot_cap, int32_t* slots_used, void* stream);
int ifx_attn_merge_partials(const void* workspace, int32_t slot_cap, int32_t slots_used, ifx_bf16* out, float* lse,
                            int32_t q_rows, int32_t heads, void* stream);

/* Merge two partial attention results over disjoint key sets (split-KV / context
 * parallel).  Replaces update_out_and_lse_pass_q
 * (inferix/models/attention/distributed.py:30-48).
 *   out_a/out_b [rows, heads, 128] bf16, lse_a/lse_b [heads, rows] fp32;
 *   result written to out_a / lse_a. */
int ifx_lse_merge(ifx_bf16* out_a, float* lse_a, const ifx_bf16* out_b, const float* lse_b,
                  int32_t rows, int32_t heads, void* stream);

/* ------------------------------------------------------------------------
 * Fused QK-RMSNorm + 3-axis RoPE + KV append.
 * Replaces, per layer: WanRMSNorm on q and k over ALL channels
 * (inferix/models/wan_base/components.py:107-126, applied causal_model.py:172-173),
 * causal_rope_apply[_chunked] (causal_model.py:33-100) and the cache write
 * causal_model.py:303-304 (+ the manager round trip :416-441).
 *
 *   qkv      : [rows, 3*dim] bf16 — fused q|k|v projection output (bias included)
 *   q_out    : [rows, dim] bf16   — RMSNorm(q)*wq then RoPE
 *   K slot(local_start + r) <- RoPE(RMSNorm(k)*wk),  V slot <- v   (via kv page table)
 *   rope     : position tables + token grid (NULL = no rotation: cross-attn q)
 *   kv       : NULL = no append (cross-attention query path)
 * Row r of this rank is token (frame r / hw_local, hw index hw_offset + r % hw_local):
 * temporal position start_frame + frame, height (hw / width), width (hw % width) — the
 * single-GPU case is hw_offset = 0, hw_local = height*width; the context-parallel case
 * is the reference's per-frame hw slice (causal_model.py:64-100,939-942).
 * Pairs are adjacent channels (2i, 2i+1); per head the head_dim/2 complex pairs split
 * [c-2*(c/3) temporal | c/3 height | c/3 width] (causal_model.py:34-37).
 * Rounding: y = bf16(x * rsqrt(mean(x^2)+eps)) ; y = bf16(y * w) ; rotation in fp64 ; bf16.
 * qkv_row_stride (elements, % 8) covers the columns read, else IFX_EINVAL: >= dim without a cache view, >= 3*dim with one,
 * >= 2*dim when the V rows are in place (flags bit 0).
 * ---------------------------------------------------------------------- */
typedef struct {
  const double* freqs;   /* device [max_pos, head_dim/2, 2] = (cos, sin): the reference's
                            complex128 `self.freqs` (causal_model.py:636-641) viewed as real */
  int32_t max_pos;       /* 1024 */
  int32_t start_frame;   /* current_start // frame_seqlen (causal_model.py:255-256) */
  int32_t height, width; /* patch grid of one frame */
  int32_t hw_offset;     /* rank * hw_local; >= 0 */
  int32_t hw_local;      /* height*width / world_size; hw_offset + hw_local <= height*width (else IFX_EINVAL) */
  float q_scale;         /* ifx_rmsnorm_rope_kv_append only: the rotated q is multiplied by this in fp32 before its single rounding
                            to bf16 (0 = 1 = the reference's q).  With q_scale = softmax_scale * log2(e) and the attention entry
                            points called with scale = ln 2 the attention is the same function of the unrounded q — q·k·scale —
                            and the self-attention kernel takes its exponent fast path (scores are exp2 arguments; no scale-FMA
                            per score).  K / V and the cache are untouched. */
  int32_t flags;         /* ABI 0.6, ifx_rmsnorm_rope_kv_append only: bit 0 = the V rows of this block are ALREADY in their cache slots
                            (written by the projection, ifx_epilogue.y2): normalise / rotate / store q and K only */
} ifx_rope_grid;

int ifx_rmsnorm_rope_kv_append(const ifx_bf16* qkv, int32_t qkv_row_stride, ifx_bf16* q_out,
                               const ifx_bf16* wq, const ifx_bf16* wk, const ifx_rope_grid* rope,
                               const ifx_kv_view* kv, int32_t local_start, int32_t rows,
                               int32_t dim, float eps, void* stream);

/* RMSNorm only, in place or out of place, [rows, dim] (cross-attention q / text K).  Row strides in elements, % 8 and >= dim
 * (else IFX_EINVAL). */
int ifx_rmsnorm(const ifx_bf16* x, int32_t x_row_stride, ifx_bf16* y, int32_t y_row_stride,
                const ifx_bf16* w, int32_t rows, int32_t dim, float eps, void* stream);

/* ------------------------------------------------------------------------
 * LayerNorm (+ AdaLN modulation).  Replaces WanLayerNorm
 * (components.py:129-142) and the per-frame modulation
 * `norm(x).unflatten(1,(F,fs)) * (1 + e[scale]) + e[shift]`
 * (causal_model.py:433,451-452,514).
 *   mode IFX_LN_PLAIN    : y = bf16(LN(x))
 *   mode IFX_LN_AFFINE   : y = bf16(LN(x) * gamma + beta)                 (norm3)
 *   mode IFX_LN_MODULATE : y = bf16(bf16(bf16(LN(x)) * bf16(1 + s)) + t), s/t = rows of `mod`
 *   mod : [groups, mod_slots, dim] bf16 = (modulation + e0) of this layer;
 *         row r uses group r / rows_per_group; shift_slot/scale_slot select the chunk.
 * Widths: dim % 8 == 0 up to 5120, and 5632 and 6144 (the 12-chunk kernel of MAGI-24B's hidden size; whole 512-column chunks only
 * above 5120).  Other widths: IFX_EUNSUP.  The same holds for ifx_layernorm_quant and ifx_layernorm_quant_static.
 * ---------------------------------------------------------------------- */
enum { IFX_LN_PLAIN = 0, IFX_LN_AFFINE = 1, IFX_LN_MODULATE = 2 };
int ifx_layernorm(const ifx_bf16* x, ifx_bf16* y, int32_t rows, int32_t dim, float eps, int32_t mode,
                  const ifx_bf16* gamma, const ifx_bf16* beta, const ifx_bf16* mod,
                  int32_t mod_slots, int32_t shift_slot, int32_t scale_slot, int32_t rows_per_group,
                  void* stream);

/* ------------------------------------------------------------------------
 * bf16 linear layer  y = epilogue(x @ W^T + bias)  on MFMA, fp32 accumulate.
 * Replaces nn.Linear calls of the block (causal_model.py:125-128,171-175,332-333,377-379,
 * wan_base/model.py:66-100) together with the elementwise ops that follow them.
 *   x [M, K] bf16 (row stride ldx), W [N, K] bf16 (nn.Linear layout), bias [N] bf16 or NULL,
 *   y [M, N] bf16 (row stride ldy).
 *   K % 64 == 0, N % 4 == 0, ldx % 8 == 0, ldy % 4 == 0, ld_res % 4 == 0 (else IFX_EINVAL).  Base pointers: x and W 16-byte aligned;
 *   y, bias, residual and mod 8-byte aligned (else IFX_EINVAL).  A launch with N, ldy or ld_res % 8 == 4, or with y, residual or mod
 *   not 16-byte aligned, runs the register-staged 128x128 kernel (8-byte epilogue vectors) whatever gemm_variant asks for.
 *   y may be the residual itself (the in-place residual of the T5 encoder layers: same base, ldy == ld_res).
 *   IFX_EPI_BIAS      : y = bf16(acc + b)
 *   IFX_EPI_GELU_TANH : y = bf16(gelu_tanh(bf16(acc + b)))                   (ffn.0 + GELU)
 *   IFX_EPI_RESIDUAL  : y = bf16(res + bf16(acc + b))                         (cross-attn o)
 *   IFX_EPI_GATE_RES  : y = bf16(res + bf16(bf16(acc + b) * gate[r / rows_per_group]))
 *                       gate = rows of `mod` [groups, mod_slots, N] at gate_slot   (:444,455-456)
 *   IFX_EPI_GELU_ERF  : y = bf16(gelu_erf(bf16(acc + b)))   exact GELU, MAGI CustomMLP fc1 (magi/dit/dit_module.py:545-557)
 * ---------------------------------------------------------------------- */
enum { IFX_EPI_BIAS = 0, IFX_EPI_GELU_TANH = 1, IFX_EPI_RESIDUAL = 2, IFX_EPI_GATE_RES = 3, IFX_EPI_GELU_ERF = 4 };
typedef struct {
  int32_t epilogue;
  const ifx_bf16* residual;  /* [M, N], row stride ld_res */
  int32_t ld_res;
  const ifx_bf16* mod;       /* [groups, mod_slots, N] */
  int32_t mod_slots;
  int32_t gate_slot;
  int32_t rows_per_group;
  /* ABI 0.6 — second destination (zero-initialised = off): output columns [split_col, N) go to y2 [M, N - split_col] (row stride
   * ldy2, 16-byte aligned, ldy2 % 8 == 0) instead of y.  The block's fused q|k|v projection writes its V columns straight into the
   * rows of the KV cache that way (a contiguous cache: y2 = v + local_start * dim) and ifx_rmsnorm_rope_kv_append is told not to copy
   * them (ifx_rope_grid.flags).  split_col must be a multiple of 256; served by the persistent ping-pong tiles only (launches of
   * >= 2048 rows, bf16, IFX_EPI_BIAS): any other launch with y2 set returns IFX_EINVAL rather than dropping the columns. */
  ifx_bf16* y2;
  int32_t ldy2;
  int32_t split_col;
} ifx_epilogue;
int ifx_gemm_bf16(const ifx_bf16* x, int32_t ldx, const ifx_bf16* w, const ifx_bf16* bias,
                  ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K,
                  const ifx_epilogue* epi, void* stream);

/* ifx_gemm_bf16 with a caller-provided scratch buffer, which lets the library pick tiles that split K between workgroups (the
 * four-wave 256 x 256 tile with two K halves for long-K launches whose tiles would fill less than half of the chip: the FFN
 * down-projection of the block, 4680 x 1536 x 8960).  ifx_gemm_workspace_bytes returns what a shape wants (0 = none: the call is
 * then identical to ifx_gemm_bf16).  The FIRST 4096 bytes of the workspace must be zero on entry (zero it once after allocation);
 * every call leaves them zero.  Launches that share a workspace must be ordered on one stream.  Results are deterministic
 * (a + b == b + a for the two partial sums). */
int64_t ifx_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K);
int ifx_gemm_bf16_ws(const ifx_bf16* x, int32_t ldx, const ifx_bf16* w, const ifx_bf16* bias, ifx_bf16* y, int32_t ldy,
                     int32_t M, int32_t N, int32_t K, const ifx_epilogue* epi, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------
 * Dynamic 8-bit linear layers: per-token activation x per-channel weight, FP8 (OCP e4m3fn) or INT8.
 * Replaces the DAX `quantize_dynamic` linears wired in
 * example/quantization/run_self_forcing_quantized.py:19-23,47-64 (every nn.Linear under generator.model
 * except text_embedding / proj_out / head).  DAX is un-vendored and unpinned: the arithmetic is defined HERE
 * (restated in oracle/quant_oracle.py); parity with DAX itself is unpinned.
 *
 *   ifx_quant_per_token : s[m] = max_k|x[m,k]| / QMAX (1.0 for a zero row), QMAX = 448 | 127;
 *                         q[m,k] = cast(clamp(x[m,k] / s[m], +-QMAX)), e4m3: RNE, int8: rint.
 *                         x [rows, K] bf16 (row stride ldx), q [rows, K] bytes (row stride ldq), scale [rows] fp32;
 *                         ldx, ldq % 8 and >= K (else IFX_EINVAL).
 *   ifx_gemm_q8         : y = epilogue(bf16(acc * (x_scale[m] * w_scale[n]) + bias[n])), acc = sum_k xq*wq in
 *                         fp32 (fp8 MFMA) or exact int32 (int8 MFMA); wq [N, K] bytes, w_scale [N] fp32 from the
 *                         same rule applied per output channel.  Epilogues as ifx_gemm_bf16.  K % 128 == 0, N % 4 == 0,
 *                         ldx % 16 == 0, ldy % 4 == 0 (else IFX_EINVAL).  Base pointers: xq, wq and w_scale 16-byte aligned; y,
 *                         bias, residual and mod 8-byte aligned (else IFX_EINVAL); N, ldy, ld_res % 8 == 4 or a y / residual /
 *                         mod that is not 16-byte aligned runs the register-staged kernel, as in ifx_gemm_bf16.
 *                         ifx_gemm_q8_ws and ifx_gemm_q8_quant_out check the same (yq 8-byte aligned: the LDS-DMA tiles
 *                         store eight e4m3 bytes at a time).
 * ---------------------------------------------------------------------- */
enum { IFX_Q_FP8_E4M3 = 0, IFX_Q_INT8 = 1 };
int ifx_quant_per_token(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, float* scale, int32_t rows,
                        int32_t K, int32_t format, void* stream);
int ifx_gemm_q8(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                const ifx_bf16* bias, ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K, int32_t format,
                const ifx_epilogue* epi, void* stream);
/* ifx_gemm_q8 with a caller-provided scratch buffer (the contract of ifx_gemm_bf16_ws: first 4096 bytes zero on entry and on exit,
 * one stream per workspace): long-K, narrow-N launches — the block's FFN down-projection, 4680 x 1536 x 8960: 114 tiles of 256 x 256
 * for 256 CUs — then run the 256-token ping-pong tile with K split between two workgroups.  Which shapes split is a function of N
 * and K only (a row's bits do not depend on the launch's row count); e4m3: first half + second half in fp32, int8: the two exact
 * int32 sums are added as integers — the same bits as the unsplit launch.  ifx_gemm_q8_workspace_bytes: what a shape wants (0 = none).
 * e4m3 BIT STABILITY: "a row's bits do not depend on the launch" holds when every launch of a shape goes through THIS entry
 * point with the workspace it asks for — what inferix_amd does.  A launch of a split shape runs UNSPLIT (first + second K half summed
 * in one fp32 chain instead of two: e4m3 results may differ in a few elements per million, int8 results never) when: the caller uses
 * plain ifx_gemm_q8 or passes no / too small a workspace; the gate epilogue has rows_per_group < 128; ifx_gemm_q8_quant_out (static
 * output quantiser) is used; bias / residual / gate / scale pointers or ldx miss the tile's alignment (8 / 16 bytes, ldx % 16); the
 * launch has more than 1024 tiles of 256 x 256 (M > ~43 000 at N = 1536); or gemm_variant forces another tile. */
int64_t ifx_gemm_q8_workspace_bytes(int32_t M, int32_t N, int32_t K);
int ifx_gemm_q8_ws(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale, const ifx_bf16* bias,
                   ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K, int32_t format, const ifx_epilogue* epi,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* ifx_layernorm_quant: ifx_layernorm followed by ifx_quant_per_token of its bf16 result, in one pass over the row — what the
 * quantised qkv / cross-attention q / ffn.0 linears of a block see (the reference's DAX wrapper quantises the input of every
 * nn.Linear, i.e. the norm's bf16 output: run_self_forcing_quantized.py:47-64, causal_model.py:419-428,470-476).  Same bytes and
 * scales as the two calls, bit for bit; the bf16 row is not written.  Arguments as ifx_layernorm + (q, ldq, scale, format). */
int ifx_layernorm_quant(const ifx_bf16* x, void* q, int32_t ldq, float* scale, int32_t rows, int32_t dim, float eps,
                        int32_t mode, const ifx_bf16* gamma, const ifx_bf16* beta, const ifx_bf16* mod, int32_t mod_slots,
                        int32_t shift_slot, int32_t scale_slot, int32_t rows_per_group, int32_t format, void* stream);

/* ifx_gemm_q8_quant_out: ifx_gemm_q8 with a GELU epilogue (IFX_EPI_GELU_TANH / IFX_EPI_GELU_ERF) whose bf16 result goes straight through
 * ifx_quant_static's rule instead of to memory: yq[m, n] = e4m3(div_clamp_to(gelu(bf16(acc * scales + bias)), out_divisor[n])), bytes at
 * yq + m * ldyq + n (ldyq in BYTES, % 8).  It is fc1 -> fc2 of MAGI's fp8_quant MLP (CustomMLP, dit_module.py:493-560: the input of the
 * PerChannelQuantizedFp8Linear fc2 is fc1's activation divided by smooth_scale): same bytes as ifx_gemm_q8 + ifx_quant_static, bit for
 * bit, without the [rows, ffn] bf16 round trip.  N % 8 == 0.
 * ifx_layernorm_quant_static: ifx_layernorm (plain / affine) followed by n_out ifx_quant_static passes of its bf16 row, each with its own
 * per-input-channel divisor vector (divisors [n_out][dim] fp32): output j lands at byte column j * dim of q (row stride ldq >= n_out *
 * dim bytes).  MAGI's q / qx / k / v linears quantise the same normalised row with their own input_scale vectors (:448-462). */
int ifx_gemm_q8_quant_out(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                          const ifx_bf16* bias, void* yq, int32_t ldyq, int32_t M, int32_t N, int32_t K, int32_t format,
                          const ifx_epilogue* epi, const float* out_divisor, int32_t via_bf16, void* stream);
int ifx_layernorm_quant_static(const ifx_bf16* x, void* q, int32_t ldq, const float* divisors, int32_t n_out, int32_t rows,
                               int32_t dim, float eps, int32_t mode, const ifx_bf16* gamma, const ifx_bf16* beta,
                               int32_t via_bf16, void* stream);

/* Static-scale and per-tensor quantisers (the other qconfig families north_star names, and MAGI's own FP8 linears).
 *   ifx_quant_static     : q[m,k] = cast(clamp(x[m,k] / divisor[k or 0], +-QMAX)).  With via_bf16 = 1 the clamped quotient is
 *                          rounded to bf16 before the e4m3 cast — exactly `div_clamp_to`, the one quantisation routine in the
 *                          reference tree (inferix/models/magi/dit/dit_module.py:367-387), used by PerTensorQuantizedFp8Linear
 *                          (divisor = input_scale [in_features], :448-462) and PerChannelQuantizedFp8Linear (divisor =
 *                          smooth_scale [1, in_features], :480-490).  divisor_len = K (per input channel) or 1.  row_scale:
 *                          optional [rows] fp32, filled with divisor[0] when divisor_len == 1 (feeds ifx_gemm_q8's x_scale).
 *                          The matmul itself is flashinfer's bmm_fp8 upstream (un-vendored): ifx_gemm_q8 with x_scale[m] =
 *                          input_scale and w_scale[n] = weight_scale computes bf16(acc * (input_scale * weight_scale)).
 *   ifx_quant_per_tensor : dynamic per-TENSOR scale s = max|x| / QMAX (1.0 for an all-zero tensor), q = cast(clamp(x / s)),
 *                          row_scale[m] = s for every row.  Two kernels on the stream (abs-max reduction into the 4-byte
 *                          amax_workspace, which the call zeroes with hipMemsetAsync, then the quantiser); no host sync.
 *   Both: K % 8 == 0; ldx (elements) and ldq (bytes) >= K and % 8 — a row stride below K is refused (rows would overlap). */
int ifx_quant_static(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, const float* divisor, int32_t divisor_len,
                     float* row_scale, int32_t rows, int32_t K, int32_t format, int32_t via_bf16, void* stream);
int ifx_quant_per_tensor(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, float* row_scale, void* amax_workspace,
                         int32_t rows, int32_t K, int32_t format, void* stream);

/* ------------------------------------------------------------------------
 * KV cache maintenance.  ifx_kv_roll: the reference's eviction shift
 * cache[sink : sink+rolled] <- cache[sink+evicted : sink+evicted+rolled]
 * (causal_model.py:287-292) as a physical move, for spans that are not page aligned
 * (page-aligned spans are handled by rotating the page table on the host). */
int ifx_kv_roll(const ifx_kv_view* kv, int32_t sink_tokens, int32_t evicted, int32_t rolled,
                ifx_bf16* scratch, void* stream);

/* Sequence-parallel cache write (the "cache write post-a2a" of CoreAttention.forward,
 * inferix/models/attention/distributed.py:183-208, for the replicated-cache design of DESIGN.md §6): the
 * all-gathered K/V rows of the new block, rank-major
 *   gathered [world][2 (K,V)][frames*hw_local][kv_heads*128] bf16,
 * go to the cache slots of logical tokens local_start + f*frame_tokens + r*hw_local + i, i.e. the single-GPU
 * (frame, hw) order of causal_model.py:939-942 / 1008-1022, through the page table when there is one. */
int ifx_kv_scatter_shards(const ifx_bf16* gathered, int32_t world, int32_t frames, int32_t hw_local,
                          int32_t frame_tokens, int32_t local_start, const ifx_kv_view* kv, void* stream);

/* Sequence-parallel exchange WITHOUT a collective: every rank stores its post-RoPE K and raw V rows of the new block
 * straight into the cache slots of every peer's replicated KV cache over xGMI.  Stands where the reference has the Ulysses
 * all-to-all + ring p2p of inferix/models/attention/distributed.py:183-208,610-706 (and where this library's first design had one
 * all-gather + ifx_kv_scatter_shards per layer).
 *   ifx_peer_alloc / _free     device memory other processes can map (fine_grained != 0: visible to running kernels — flag blocks)
 *   ifx_peer_export / _open / _close   64-byte HIP IPC handle of the allocation `ptr` lies in + the offset of `ptr` in it  <->  the
 *                              allocation's base mapped into this process (add the offset)
 *   ifx_rmsnorm_rope_kv_push   rows [rows, >= 2*dim] = (k | v) of the K/V-only projection: K <- RoPE(RMSNorm(k) * wk), V raw, row r
 *                              (f = r / slot_hw_local, i = r % slot_hw_local) stored at the slot of logical token
 *                              local_start + f*frame_tokens + slot_hw_offset + i of EVERY destination (same page table / segment map
 *                              everywhere: `geometry` gives it, its k/v pointers are ignored).  One destination = the rank's own cache
 *                              or staging buffer: the K/V-only form of ifx_rmsnorm_rope_kv_append.
 *   ifx_peer_signal            flags[p][index] <- value in every peer's flag block, stream-ordered, released at system scope
 *   ifx_peer_wait              stream-ordered wait until flags[i] >= value for i < count (this rank's own block); after timeout_ms
 *                              the kernel gives up and stores 1 + i into *status (host checks it at a synchronisation point). */
#define IFX_MAX_PEERS 8
#define IFX_PEER_HANDLE_BYTES 64
typedef struct {
  int32_t count;
  ifx_bf16* k[IFX_MAX_PEERS];
  ifx_bf16* v[IFX_MAX_PEERS];
} ifx_peer_caches;
typedef struct {
  int32_t count;
  int32_t* flags[IFX_MAX_PEERS];
} ifx_peer_flags;
int ifx_peer_alloc(int64_t bytes, int32_t fine_grained, void** ptr);
int ifx_peer_free(void* ptr);
int ifx_peer_export(const void* ptr, uint8_t* handle, int64_t* offset);
int ifx_peer_open(const uint8_t* handle, void** ptr);
int ifx_peer_close(void* ptr);
int ifx_rmsnorm_rope_kv_push(const ifx_bf16* kv_rows, int32_t kv_row_stride, const ifx_bf16* wk, const ifx_rope_grid* rope,
                             const ifx_peer_caches* peers, const ifx_kv_view* geometry, int32_t local_start, int32_t frame_tokens,
                             int32_t slot_hw_local, int32_t slot_hw_offset, int32_t rows, int32_t dim, float eps, void* stream);
int ifx_peer_signal(const ifx_peer_flags* peers, int32_t index, int32_t value, void* stream);
int ifx_peer_wait(const int32_t* flags, int32_t count, int32_t value, int32_t timeout_ms, int32_t* status, void* stream);

/* ----------------------------------------------------------------------
 * VAE decoder: channels-last causal 3-D convolution.
 * Replaces CausalConv3d.forward + the feature-cache concatenation around it
 * (inferix/models/wan_base/vae.py:26-34, 207-216), the nearest-2x Upsample +
 * Conv2d of Resample (vae.py:58-64, 83-90, 139-141) and the residual add of
 * ResidualBlock.forward (vae.py:219).
 *   x          frames [slot][hs][ws][cin] bf16; logical input frame f (0 .. t_out+kt-2: for kt = 3 the two
 *              history frames, then the new ones) lives at x + in_slots[f] * in_frame_stride; in_slots[f] < 0
 *              = an all-zero frame (the causal padding in front of the stream)
 *   in_planar  1: the input frames are [cin/32][hs][ws][32] instead (32-channel planes: the halo patch of one
 *              channel chunk is then rows of contiguous 64-byte pixels — LDS-DMA moves 64-byte rows that lie
 *              192+ bytes apart at a third of the rate of contiguous ones, round 6; the frame rings in front of
 *              the 3x3x3 convs use this layout, written by ifx_rmsnorm_cl with IFX_NORM_OUT_PLANAR)
 *   upsample   1: the 3x3 taps read the nearest-2x upsampled frame (output 2hs x 2ws), never materialised
 *   w          [kt*ks*ks][cin/32][cout][32] bf16: tap-major, 32-channel-chunk-major repack of the torch
 *              [cout][cin][kt][ks][ks] weight (a DMA piece of 16 output channels x 32 input channels is contiguous)
 *   y          output frame t at y + out_slots[t] * out_frame_stride, [ho][wo][cout]
 *   residual   NULL or contiguous [t_out][ho][wo][cout]: y = bf16(bf16(conv + bias) + residual)
 *   zero_page  >= 64 bytes of zeros in device memory
 * in_slots / out_slots are HOST arrays (copied into the launch).
 * Alignment (the kernels move 16 bytes per lane; a call that breaks a rule is refused with IFX_EINVAL, nothing is launched):
 *   x and w are 16-byte aligned and in_frame_stride is a multiple of 8 elements, always;
 *   when cout % 8 == 0, y and residual are 16-byte aligned and out_frame_stride is a multiple of 8 elements (other
 *   channel counts are stored, and their residual read, element by element: any out_frame_stride, 2-byte alignment).
 * ---------------------------------------------------------------------- */
typedef struct {
  const ifx_bf16* x;
  int64_t in_frame_stride;      /* elements */
  const int32_t* in_slots;
  int32_t hs, ws, cin, upsample;
  const ifx_bf16* w;
  const ifx_bf16* bias;         /* [cout] or NULL */
  int32_t kt, ks;               /* temporal 1|3, spatial 1|3 */
  ifx_bf16* y;
  int64_t out_frame_stride;     /* elements */
  const int32_t* out_slots;
  int32_t cout, t_out;
  const ifx_bf16* residual;
  const void* zero_page;
  int32_t in_planar;            /* ABI minor 7; 0 = channels-last input frames */
} ifx_conv3d_desc;
int ifx_conv3d_cl(const ifx_conv3d_desc* desc, void* stream);

/* Per-pixel channel RMS norm (+ SiLU) of channels-last frames x [frames][frame_pixels][channels], with the bf16 op
 * chain of RMS_norm.forward (vae.py:52-55) and nn.SiLU; frame f is written to y + out_slots[f] * out_frame_stride
 * (the ring buffer that holds the next conv's input and its two-frame history).  out_slots is a HOST array.
 * flags: IFX_NORM_SILU (1) applies SiLU; IFX_NORM_OUT_PLANAR (2; channels % 32 == 0) writes the frame as
 * [channels/32][frame_pixels][32] (ifx_conv3d_desc.in_planar) instead of channels-last. */
#define IFX_NORM_SILU 1
#define IFX_NORM_OUT_PLANAR 2
int ifx_rmsnorm_cl(const ifx_bf16* x, const ifx_bf16* gamma, ifx_bf16* y, int64_t out_frame_stride,
                   const int32_t* out_slots, int32_t frames, int32_t frame_pixels, int32_t channels,
                   int32_t flags, void* stream);

/* probs = softmax(scores * scale) row-wise, bf16 [rows][ld] (single-head attention of the VAE middle block,
 * vae.py:250-254, between the two ifx_gemm_bf16 launches that form QK^T and PV). */
int ifx_softmax_rows(const ifx_bf16* scores, ifx_bf16* probs, int32_t rows, int32_t cols, int32_t ld, float scale,
                     void* stream);

/* Frame finishing of the streaming path: n bf16 pixels in [-1, 1] (the decoder's channels-last output, which is already the
 * frame layout [t][h][w][3]) -> n uint8.  Per element, in fp32:
 *   f = clamp(float(x), -1, 1);  g = clamp(f * 0.5 + 0.5, 0, 1);  y = (uint8)clamp(g * 255, 0, 255)   (truncating)
 * — bit for bit the chain decode_to_pixel(...).float().clamp_(-1, 1) -> (v * 0.5 + 0.5).clamp(0, 1) -> clamp(v * 255, 0, 255)
 * .to(uint8) that the per-block streaming callback runs in six fp32 passes.  +-inf clamp like any value; the result for a NaN is
 * unspecified.  x needs 2-byte alignment only and y none (16-byte loads behind a scalar head; 8-byte stores where y is aligned
 * with x, byte stores otherwise).  n == 0 is IFX_OK without a launch; a null pointer or n < 0 is IFX_EINVAL.
 * (New export: no ABI bump.) */
int ifx_frames_u8(const ifx_bf16* x, uint8_t* y, int64_t n, void* stream);

/* YUV 4:2:0 frames finished on the device: what a video encoder takes (yuv420p / nv12), defined in integers so that every byte is.
 * R, G, B are uint8: for ifx_frames_yuv420 the values ifx_frames_u8 gives for the bf16 pixels x [t][h][w][3] (the same fp32 chain),
 * for ifx_rgb8_yuv420 the bytes of x [t][h][w][3] as they are.  With m (row-major 3 x 3) and a from the descriptor:
 *   luma, per pixel:          Y  = clamp255((m[0] R + m[1] G + m[2] B + a[0]) >> 8)
 *   chroma, per 2 x 2 quad:   R' = (R00 + R01 + R10 + R11 + 2) >> 2, likewise G', B'   (a box filter: chroma sits at the quad's centre)
 *                             Cb = clamp255((m[3] R' + m[4] G' + m[5] B' + a[1]) >> 8)
 *                             Cr = clamp255((m[6] R' + m[7] G' + m[8] B' + a[2]) >> 8)
 * a carries the rounding term and the bias (128 + 16 << 8 = 4224 for limited-range luma, 128 + 128 << 8 = 32896 for chroma), so the
 * sums of a sensible matrix are non-negative; >> is arithmetic and clamp255 clamps to 0 .. 255 on both sides.  The caller owns the
 * matrices (BT.601 / BT.709, limited / full range: inferix_amd/hip_ops.py YUV420_PRESETS); there is one kernel body.
 * One frame of y is h w 3 / 2 contiguous bytes, frames back to back:
 *   IFX_YUV420_I420   Y [h][w], U [h/2][w/2], V [h/2][w/2]              (PyAV's yuv420p ndarray, [h 3/2][w])
 *   IFX_YUV420_NV12   Y [h][w], UV [h/2][w] with U, V interleaved
 * h and w must be even (IFX_EINVAL otherwise, the message names the size), as are a null pointer, a negative t, h or w and an unknown
 * layout; t == 0 (or an empty frame) is IFX_OK without a launch.  x needs its element's alignment only and y none: with w % 8 == 0,
 * x 16-byte (bf16) / 8-byte (uint8) aligned and y 8-byte aligned a lane takes 2 rows x 8 columns with vector accesses, otherwise one
 * quad with scalar ones.  The result for a NaN is unspecified, as for ifx_frames_u8.  (New exports: no ABI bump.) */
#define IFX_YUV420_I420 0
#define IFX_YUV420_NV12 1
typedef struct ifx_yuv420_desc {
  int32_t m[9]; /* row-major: Y row, Cb row, Cr row, in 1/256 */
  int32_t a[3]; /* per row: rounding term + bias, in 1/256 */
} ifx_yuv420_desc;
int ifx_frames_yuv420(const ifx_bf16* x, uint8_t* y, int32_t t, int32_t h, int32_t w, int32_t layout, const ifx_yuv420_desc* coeffs,
                      void* stream);
int ifx_rgb8_yuv420(const uint8_t* x, uint8_t* y, int32_t t, int32_t h, int32_t w, int32_t layout, const ifx_yuv420_desc* coeffs,
                    void* stream);

/* ----------------------------------------------------------------------
 * umT5 text encoder.
 * ifx_t5_attention: bidirectional self-attention of T5Attention.forward between its q/k/v and o linears
 * (inferix/models/wan_base/text_encoder/t5.py:96-117), head_dim 64, NO 1/sqrt(d) scaling:
 *   s = bf16(bf16(q.k) + bias[h][key - query]) ; keys >= seq_lens[b] get finfo(bf16).min ; p = bf16(softmax_fp32(s)) ;
 *   out = bf16(p v).
 *   q/k/v/out   rows b*seq_len_padded + t, channels h*64 + c, given row strides (q, k, v may be the column blocks of one
 *               fused qkv GEMM output)
 *   rel_bias    [heads][2*seq_len_padded - 1] bf16: the T5RelativeEmbedding value (t5.py:235-266) of relative offset
 *               (key - query) at index offset + seq_len_padded - 1; the [1, heads, L, L] tensor is never built
 *   seq_lens    [batch] int32 in device memory
 * seq_len_padded in [32, 512], multiple of 32 (K and V^T of one head are staged in LDS).
 * ---------------------------------------------------------------------- */
int ifx_t5_attention(const ifx_bf16* q, int32_t ldq, const ifx_bf16* k, int32_t ldk, const ifx_bf16* v, int32_t ldv,
                     ifx_bf16* out, int32_t ldo, const ifx_bf16* rel_bias, const int32_t* seq_lens, int32_t batch,
                     int32_t seq_len_padded, int32_t heads, void* stream);

/* h[rows][ffn] = fc1 * GELU(gate) with the tanh GELU of t5.py:50-52 evaluated op by op in bf16 (T5FeedForward.forward,
 * t5.py:138-139); gate_fc1 = [rows][2*ffn], columns [0, ffn) = gate pre-activation, [ffn, 2 ffn) = fc1 (one fused GEMM). */
int ifx_t5_gated_gelu(const ifx_bf16* gate_fc1, ifx_bf16* h, int32_t rows, int32_t ffn, void* stream);

/* ----------------------------------------------------------------------
 * fp32 T5 v1.1 caption encoder of MAGI-1: HuggingFace `T5EncoderModel` as `T5Embedder` runs it, torch_dtype=torch.float
 * (inferix/models/magi/t5/t5_model.py:126, 145-149; inferix/pipeline/magi/prompt_process.py:135-144).  Every operand and result is
 * fp32; nothing in the chain is rounded to a narrower format.  Additive exports: IFX_ABI_MINOR is unchanged.
 *
 * ifx_gemm_f32: y[M][N] = x[M][K] . w[N][K]^T (+ res[M][N]) — the bias-free nn.Linear of T5Attention q / k / v / o and of
 * T5DenseGatedActDense wi_0 / wi_1 / wo, with the residual add of T5LayerSelfAttention / T5LayerFF.
 *   x, y, res   row strides ldx, ldy, ld_res in elements (x may be a column block of a wider matrix; y may be res itself)
 *   w           [N][K] contiguous
 *   tile        0 = chosen by M and N, 1 = the 128-row tile, 2 = the 32-row tile
 * K % 64 == 0, N % 64 == 0, any M >= 1, x and w 16-byte aligned with ldx % 4 == 0: anything else is IFX_EUNSUP, nothing is launched.
 * v_mfma_f32_32x32x2_f32 with ONE accumulation chain per output element, in k order 0 .. K-1, the residual added last (no split-K,
 * no atomics): a row's result is bitwise independent of M and of the tile that ran.
 * ---------------------------------------------------------------------- */
int ifx_gemm_f32(const float* x, int32_t ldx, const float* w, const float* res, int32_t ld_res, float* y, int32_t ldy, int32_t M,
                 int32_t N, int32_t K, int32_t tile, void* stream);
/* The middle of HF T5Attention.forward for an encoder, head size 64, NO 1/sqrt(d) scaling: per (prompt, head)
 *   s = q.k + rel_bias[h][key - query] ; keys >= seq_lens[b] get probability exactly 0 and are never read ; p = softmax_fp32(s) ;
 *   out = p v.
 *   q/k/v/out       rows b*seq_len_padded + t, channels h*64 + c, row strides % 4 (the column blocks of one fused qkv output)
 *   rel_bias        [heads][2*seq_len_padded - 1] fp32, offset (key - query) at index offset + seq_len_padded - 1; ONE table for
 *                   every layer (only block 0 owns relative_attention_bias)
 *   seq_lens        [batch] int32 in device memory; 0 writes zeros
 *   seq_len_padded  any multiple of 8 in [8, 1024]
 *   query_rows      0: every padded row is computed, as HF does; 1: rows < seq_lens[b] only, zeros in the rest (those q rows are
 *                   not read).  Valid rows are bitwise the same in both modes. */
int ifx_t5_attention_f32(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv, float* out,
                         int32_t ldo, const float* rel_bias, const int32_t* seq_lens, int32_t batch, int32_t seq_len_padded,
                         int32_t heads, int32_t query_rows, void* stream);
/* HF T5LayerNorm: y = w * (x * rsqrt(mean(x^2) + eps)).  dim a multiple of 64 up to 4096 (else IFX_EUNSUP); y may be x. */
int ifx_rmsnorm_f32(const float* x, int32_t ldx, const float* w, float* y, int32_t ldy, int32_t rows, int32_t dim, float eps,
                    void* stream);
/* h[rows][ffn] = gelu_new(g) * u of T5DenseGatedActDense, gelu_new(g) = 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3)));
 * gate_up = [rows][2*ffn] = (wi_0 x | wi_1 x) from one fused GEMM.  ffn % 4 == 0. */
int ifx_t5_gated_gelu_f32(const float* gate_up, float* h, int32_t rows, int32_t ffn, void* stream);

/* ----------------------------------------------------------------------
 * MAGI transformer layer (BASELINE config 5), the row kernels between its GEMMs and attention calls.
 *
 * ifx_magi_head_prep: everything FullyParallelAttention.get_q / get_k / get_v / get_xqkv do to the projection outputs
 * (inferix/models/magi/dit/dit_module.py:902-970), one pass over the fused projection row:
 *   layout 0: in = [rows, q_heads q | q_heads qx | kv_heads k | kv_heads v] x 128 (ONE GEMM over the concatenated
 *             linear_qkv.{q,qx,k,v} weights)
 *               q  : fp32 LayerNorm(128; qn_w (+1), qn_b) -> non-interleaved rotary (flash-attn apply_rotary_emb: with the head
 *                    split x1 | x2, out = x1*cos - x2*sin | x1*sin + x2*cos, fp32) -> bf16 -> q_out[r, h*128]
 *               k  : the same with kn_w / kn_b -> k_out[dest(r), h]
 *               v  : copy -> v_out[dest(r), h]
 *               qx : bf16 LayerNorm(xn_w (+1 in bf16), xn_b), one rounding -> qx_out[r, h*128]      (q_layernorm_xattn)
 *   layout 1: in = [rows, kv_heads x (k | v)] x 128 (linear_kv_xattn output viewed [y, hn, 2*hd], :959-968)
 *               k  : bf16 LayerNorm(xn_w, xn_b) (k_layernorm_xattn) -> k_out[dest(r), h];  v : copy -> v_out[dest(r), h]
 *   rope      [rows, 128] fp32 = (sin[64] | cos[64]) per token, the reference's rotary_pos_emb rows (:1097)
 *   k / v destination: element offset dest(r) * ld_kv + h * kv_head_stride with
 *               dest(r) = r < split ? row0 + r : row1 + (r - split)
 *             i.e. the rows MagiKVCacheManager's rule stores go to their final cache slots and the rest to the scratch tail
 *             (inferix/kvcache_manager/model/magi_kv_cache_manager.py:76-187); or (row0 = 0, split = rows) a staging buffer
 *             of the Ulysses all-to-all.
 * ---------------------------------------------------------------------- */
typedef struct {
  const ifx_bf16* in;
  int32_t ld_in, rows, layout, q_heads, kv_heads, head_dim;
  const float* rope;
  const float *qn_w, *qn_b, *kn_w, *kn_b;     /* fp32 [128] */
  const ifx_bf16 *xn_w, *xn_b;                /* bf16 [128] */
  float eps;
  int32_t layernorm_1p;                       /* apply_layernorm_1p: norm weight + 1 */
  ifx_bf16* q_out;
  int32_t ld_q;
  ifx_bf16* qx_out;
  int32_t ld_qx;
  ifx_bf16* k_out;
  ifx_bf16* v_out;
  int32_t ld_kv, kv_head_stride;
  int32_t row0, split, row1;
  float q_scale;                              /* q (self-attention queries only) is multiplied by this in fp32 before its one rounding to bf16;
                                                 0 = 1.  softmax_scale * log2(e) here + attention scale = ln 2 = the same attention on the
                                                 exponent fast path (see ifx_rope_grid.q_scale) */
  int32_t rope_half;                          /* rotary pairs per head: rope rows are [2 * rope_half] fp32 = (sin | cos), channel e < rope_half
                                                 pairs with e + rope_half and the channels behind 2 * rope_half pass through.  0 = 64 (the whole
                                                 head).  MAGI's table covers 96 of the 128 head channels (3 axes x head_dim / 8 bands,
                                                 dit_module.py:673-720): rope_half = 48.  Multiple of 8. */
  int32_t q_group;                            /* ABI 0.6, 0 = off: self-attention q head h is written at
                                                 q_out + (h / q_group) * q_group_stride + r * ld_q + (h % q_group) * 128 — the send order of
                                                 the head -> rank all-to-all ([(cp seq), heads / cp, 128]: q_group = heads / cp, ld_q = q_group *
                                                 128, q_group_stride = rows * ld_q), so that no layout copy stands between this kernel and the
                                                 collective (context_parallel.py:317-335's permute + contiguous) */
  int64_t q_group_stride;
} ifx_magi_head_prep_desc;
int ifx_magi_head_prep(const ifx_magi_head_prep_desc* desc, void* stream);

/* bias_modulate_add (dit_module.py:295-313): the Triton `range_mod_kernel_fwd` (:204-292) + post-norm + residual in one pass:
 *   y[r] = bf16( LayerNorm_fp32( float(x[r]) * float(gate[condition_map[r]]) ; norm_w (+1), norm_b ) + float(residual[r]) )
 *   gate: rows of the softcapped AdaModulateLayer output, row stride ld_gate (pass gate + hidden for the MLP half);
 *   norm_w / norm_b fp32 [dim] (self_attn_post_norm / mlp_post_norm are fp32 modules, dit_model.py:620-637). */
int ifx_magi_gate_norm_residual(const ifx_bf16* x, int32_t ldx, const ifx_bf16* residual, int32_t ld_res,
                                const int32_t* condition_map, const ifx_bf16* gate, int32_t ld_gate, const float* norm_w,
                                const float* norm_b, int32_t layernorm_1p, ifx_bf16* y, int32_t ldy, int32_t rows, int32_t dim,
                                float eps, void* stream);

/* Elementwise bf16 -> bf16 with fp32 math and one rounding: IFX_ACT_SILU (AdaModulateLayer.act, :196-198),
 * IFX_ACT_TANH (softcap with cap 1, :363-364,:1300-1303). */
enum { IFX_ACT_SILU = 0, IFX_ACT_TANH = 1 };
int ifx_act_rows(const ifx_bf16* x, ifx_bf16* y, int64_t n, int32_t mode, void* stream);
/* The activation of the gated MLP (CustomMLP with gated_linear_unit, the MAGI-24B configs; dit_module.py:528-549:
 * flashinfer.activation.silu_and_mul on the fc1 output): x [rows, 2f], gate half = columns [0, f), up half = [f, 2f), row stride ldx;
 *   y[r, j] = bf16( bf16(silu_fp32(x[r, j])) * x[r, f + j] )
 * — SiLU in fp32 rounded to bf16, the product of the two bf16 values rounded again: the chain the repository's oracle restates and
 * the reference-generated fixtures pin (oracle/magi_block_oracle.py:300-302).  flashinfer's own kernel keeps fp32 between the two
 * steps (one rounding); its source is not part of the reference tree, so that form is unpinned and not what is evaluated here.
 *   y : [rows, f] bf16, row stride ldy, or NULL.
 *   q : [rows, f] e4m3 bytes, row stride ldq (bytes), or NULL: ifx_quant_static(y, divisor, IFX_Q_FP8_E4M3, via_bf16 = 1) of the bf16
 *       result, bit for bit, without the bf16 round trip — the input of an FP8 fc2.  divisor [divisor_len] fp32, divisor_len = f (per
 *       channel) or 1; required with q, and only with q.
 * At least one of y and q.  f % 8 == 0; ldx >= 2f, ldy >= f, ldq >= f, all % 8; x, y, divisor 16-byte aligned, q 8-byte aligned.
 * rows == 0 is a no-op.  (Added without an ABI bump: a new export, no struct or signature changes.) */
int ifx_silu_and_mul(const ifx_bf16* x, int32_t ldx, ifx_bf16* y, int32_t ldy, void* q, int32_t ldq, const float* divisor,
                     int32_t divisor_len, int32_t rows, int32_t f, void* stream);
/* MagiKVCacheManager's store after the head -> rank all-to-all (inferix/models/magi/dit/dit_module.py:905-952: the K | V rows of the
 * message go into the cache, the first `split` rows to the run that is kept, the rest to the scratch run behind it):
 *   kv [rows, heads, 2 * 128] contiguous; row r -> cache row (r < split ? row0 + r : row1 + r - split) of k_cache / v_cache
 *   [slots, heads, 128] (head_dim 128).  One launch instead of four strided copies per layer. */
int ifx_kv_split_rows(const ifx_bf16* kv, ifx_bf16* k_cache, ifx_bf16* v_cache, int32_t rows, int32_t heads, int32_t row0,
                      int32_t split, int32_t row1, void* stream);

/* What `SampleTransport` does between two model forwards, in one launch: the guidance mix of `forward_dispatcher`
 * (inferix/models/magi/dit/dit_model.py:500-596) and the Euler step of `integrate` (inferix/pipeline/magi/video_generate.py:531-552)
 * on a window of n_chunks consecutive chunks of the clip latents.  For chunk c of the window and every element of it
 *   m = w0[c] * v0;   m = m + w1[c] * v1 (source 1 covers c);   m = m + w2[c] * v2 (source 2 covers c);   x = x + m * dt[c]
 * every product and sum rounded to fp32 on its own (no FMA): bit for bit the torch operator sequence.  All operands fp32.
 *   x      : the clip [rows, channels, frames, H, W], rows 1 or 2, (frames, H, W) contiguous, addressed by row_stride / chan_stride
 *            (elements); the window is frames [chunk_start * chunk_width, (chunk_start + n_chunks) * chunk_width).  With rows == 2 the
 *            result computed from row 0 is stored to both rows (the halves of the reference's guidance batch are equal).  Frames
 *            outside the window are not touched.
 *   src[i] : [channels, frames, H, W] with its own chan_stride; frame first_frame of it lies under window chunk first_chunk, and it
 *            covers window chunks first_chunk .. last_chunk (inclusive).  src[0] covers every chunk.  w[c]: its weight on chunk c.
 *   dt, w  : by value, n_chunks <= IFX_MAGI_INTEGRATE_MAX_CHUNKS (else IFX_EINVAL).
 * 16-byte accesses where x and the sources of a (channel, chunk) span share their offset from a 16-byte boundary, 4-byte ones on
 * the ragged ends and otherwise.  (New export, no change to an existing struct or signature: no ABI bump.) */
#define IFX_MAGI_INTEGRATE_MAX_CHUNKS 8
#define IFX_MAGI_INTEGRATE_MAX_SOURCES 3
typedef struct {
  const float* v;
  int64_t chan_stride;
  int32_t frames, first_frame, first_chunk, last_chunk;
  float w[IFX_MAGI_INTEGRATE_MAX_CHUNKS];
} ifx_magi_integrate_src;
typedef struct {
  float* x;
  int64_t row_stride, chan_stride;
  int32_t rows, channels, frames, frame_elems;   /* frame_elems = H * W */
  int32_t chunk_width, chunk_start, n_chunks, n_src;
  float dt[IFX_MAGI_INTEGRATE_MAX_CHUNKS];
  ifx_magi_integrate_src src[IFX_MAGI_INTEGRATE_MAX_SOURCES];
} ifx_magi_integrate_desc;
int ifx_magi_integrate(const ifx_magi_integrate_desc* desc, void* stream);

/* The copies around `VideoDiTModel`'s patch embedding (inferix/models/magi/dit/dit_model.py:111-135): latents -> the fp32 rows the
 * embedding's GEMM multiplies, in one launch instead of mul / cat / float / permute / reshape.
 *   x       : [N, C, T, H, W] fp32 or bf16 (is_bf16), dims and element strides given; the W stride must be 1, the others are free
 *             (non-negative): a frame window or a batch row of a larger tensor costs no copy.  N C <= 65535.
 *   rows    : fp32 [N * T' H' W', ld], T' = T / patch_t etc. (floor: trailing frames / rows / columns that do not fill a patch are
 *             dropped), token order (t', h', w'); column ((c pT + a) pH + b) pW + d holds x[n, c, t' pT + a, h' pH + b, w' pW + d]
 *             * scale, the order of `x_embedder.weight.reshape(hidden, -1)`.  The product is formed in x's dtype: a bf16 product is
 *             rounded to bf16 before it widens.  duplicate (half_channel_vae: `torch.cat([x, x], dim=1)`): the row is 2 C pT pH pW
 *             wide, its second half a copy of the first.  ld >= the row's width.
 * 16-byte (fp32) / 8-byte (bf16) loads along W where x, its outer strides and the kept width are multiples of four elements, else
 * one element per lane.  A null pointer, a W stride other than 1, a negative stride, an ld too small: IFX_EINVAL, nothing launched.
 * (New export, no change to an existing struct or signature: no ABI bump.) */
int ifx_magi_patch_rows(const void* x, int32_t is_bf16, const int64_t* dims, const int64_t* strides, float scale, int32_t duplicate,
                        int32_t patch_t, int32_t patch_h, int32_t patch_w, float* rows, int64_t ld, void* stream);
/* `VideoDiTModel.unpatchify` (dit_model.py:97-107) behind the final linear, with the channel cut of half_channel_vae and the division by
 * x_rescale_factor, in one launch:
 *   o   : fp32 [lat_t lat_h lat_w, batch, patch_t patch_h patch_w channels], token stride ld_token >= batch * K elements
 *   out : fp32 [batch, c_out, lat_t patch_t, lat_h patch_h, lat_w patch_w] contiguous;
 *         out[n, c, t pT + a, h pH + b, w pW + d] = o[(t H + h) W + w, n, ((a pH + b) pW + d) channels + c] / divisor for c < c_out.
 * The quotient is formed as torch's true divide by a host scalar forms it on the device — the product with 1.0f / divisor, the
 * reciprocal rounded to fp32 once on the host — so the result equals `o / x_rescale_factor` bit for bit.  16-byte stores where
 * lat_w patch_w % 4 == 0 and out is 16-byte aligned, else 4-byte ones.  A null pointer, c_out outside 1 .. channels, ld_token smaller
 * than batch * K, divisor 0: IFX_EINVAL, nothing launched.  (New export: no ABI bump.) */
int ifx_magi_unpatch(const float* o, int64_t ld_token, int32_t batch, int32_t channels, int32_t c_out, int32_t lat_t, int32_t lat_h,
                     int32_t lat_w, int32_t patch_t, int32_t patch_h, int32_t patch_w, float divisor, float* out, void* stream);

/* One step of the guided many-step causal sampler between two pairs of generator forwards, in one launch: the classifier-free-guidance
 * mix of `CausalDiffusionInferencePipeline` (inferix/pipeline/self_forcing/CausalDiffusionInferencePipeline.py:244-251) and
 * `FlowUniPCMultistepScheduler.step` (inferix/models/wan_base/utils/fm_solvers_unipc.py:655-739: conversion to x0, UniC corrector, UniP
 * predictor).  Every coefficient is a function of the sigma schedule, computed on the host (FlowUniPCSchedule.coefficients):
 *   flow   = flow_uncond + guidance * (flow_cond - flow_uncond)
 *   m_t    = x - sigma * flow
 *   x_c    = c_last * last_sample + c_m1 * m1 + c_d1 * (m2 - m1) + c_dt * (m_t - m1)     use_corrector (the c_d1 term at
 *            corrector_order 2 only);  x_c = x otherwise
 *   x_next = p_x * x_c + p_m * m_t + p_d * (m1 - m_t)                                    (the p_d term at predictor_order 2 only)
 * fp32 FMAs inside, x_next / last_out (= x_c) / m_out (= m_t) each rounded to bf16 once.  All tensors bf16.
 *   flow_cond, flow_uncond : [batch, frames, channels, H, W] addressed through (batch, frame, channel) strides in elements with a
 *                            contiguous H W plane (the model's [B, C, F, H, W] output viewed [B, F, C, H, W] is fine); every stride of
 *                            a dimension larger than 1 >= plane.
 *   x, last_sample, m1, m2, x_next, last_out, m_out : contiguous [batch, frames, channels, H, W].  last_sample, m1, m2 may be NULL
 *                            where the step does not read them (no corrector; orders 1).
 *   Allowed aliasing: x_next == x, last_out == last_sample, m_out == m2 (the history ring rotates by pointer swap): an element is
 *   read in full before its three results are stored.  Any other overlap is undefined.
 * 16-byte accesses where the nine plane starts share their offset from a 16-byte boundary, 2-byte ones on the ragged ends and
 * otherwise.  A null required pointer, an odd base address, a bad order or a stride smaller than a plane: IFX_EINVAL, nothing is
 * launched.  (New export, no change to an existing struct or signature: no ABI bump.) */
typedef struct {
  const ifx_bf16 *flow_cond, *flow_uncond;
  int64_t flow_cond_stride[3], flow_uncond_stride[3];   /* (batch, frame, channel), elements */
  const ifx_bf16 *x, *last_sample, *m1, *m2;
  ifx_bf16 *x_next, *last_out, *m_out;
  int32_t batch, frames, channels, plane;               /* plane = H * W */
  float guidance, sigma;
  float c_last, c_m1, c_d1, c_dt;
  float p_x, p_m, p_d;
  int32_t use_corrector, corrector_order, predictor_order;
} ifx_cfg_unipc_step_desc;
int ifx_cfg_unipc_step(const ifx_cfg_unipc_step_desc* desc, void* stream);

/* ----------------------------------------------------------------------
 * MAGI ViT-VAE tile decoder (BASELINE config 5, PER_BLOCK decode): what `ViTDecoder` (inferix/models/magi/vae/vae_module.py:569-716)
 * needs besides ifx_layernorm and ifx_gemm_bf16.  Head size 64 only; the other attention entry points keep refusing it.
 * (Added without an ABI bump: new exports, no struct or signature changes.)
 *
 * `Attention.forward` :281-292 between the qkv linear and the attention, IN PLACE on qkv [batch * tokens, 3 * heads * 64] (columns
 * q | k | v, each heads x 64; row stride ld):
 *   do_norm : `ManualLayerNorm` (:229-242) of every (token, q | k | v, head) - v included - in the reference's bf16 op chain:
 *             bf16(bf16(x - bf16(mean)) / bf16(bf16(std_population) + eps)), mean and std from fp32 reductions over the 64 channels
 *   do_rope : q and k of the tokens t >= cls_tokens of each tile: `apply_rot_embed` (:142-150) with the interleaved rot,
 *             out[2i] = bf16(bf16(x[2i] cos[2i]) + bf16(-x[2i+1] sin[2i])), out[2i+1] = bf16(bf16(x[2i+1] cos[2i+1]) + bf16(x[2i] sin[2i+1]));
 *             sin_table / cos_table [tokens - cls_tokens, 64] bf16, row t - cls_tokens (may be NULL without do_rope)
 * qkv and the tables 16-byte aligned, ld % 8 == 0, 3 * heads * 64 <= ld, tokens >= 1. */
int ifx_vit_head_prep(ifx_bf16* qkv, int32_t ld, const ifx_bf16* sin_table, const ifx_bf16* cos_table, int32_t batch, int32_t tokens,
                      int32_t heads, int32_t cls_tokens, int32_t do_norm, int32_t do_rope, float eps, void* stream);
/* out = softmax(q k^T / 8) v per (tile, head), non-causal, head size 64 (flash_attn_func / flash_attn_qkvpacked_func of :293-295 with
 * the default scale): q / k / v / out rows of heads x 64 channels with row strides ldq / ldk / ldv / ldo (the three column blocks of
 * the qkv buffer are fine); `batch` tiles of `tokens` consecutive rows, a tile's queries see that tile's keys only.  Any tokens >= 1:
 * rows past a tile's end are neither read nor written.  fp32 online softmax, exp(s - max) rounded to bf16 for the second product,
 * fp32 row sum, one rounding of the output.  Strides % 8 == 0 and >= heads * 64; q / k / v 16-byte, out 8-byte aligned. */
int ifx_vit_attention(const ifx_bf16* q, int32_t ldq, const ifx_bf16* k, int32_t ldk, const ifx_bf16* v, int32_t ldv, ifx_bf16* out,
                      int32_t ldo, int32_t batch, int32_t tokens, int32_t heads, void* stream);
/* `ViTDecoder.forward` :712-715 in one pass: the rearrangement 'B lT lH lW pT pH pW C -> B C (lT pT) (lH pH) (lW pW)' of the token
 * rows and the zero-padded 3 x 3 x 3 `last_layer` Conv3d(C -> 3), fp32 accumulation, one rounding:
 *   x      [batch * tile_rows, patch_t * patch_h * patch_w * channels] bf16, row stride ldx; the first cls_tokens rows of each tile
 *          are skipped, tile_rows = cls_tokens + (t_out / patch_t) (h_out / patch_h) (w_out / patch_w)
 *   weight [3, channels, 3, 3, 3] bf16, bias [3] bf16;  y [batch, 3, t_out, h_out, w_out] bf16, contiguous
 * channels == 4 (unpatch_channels of every published config); the patch sizes divide the output; ldx % 8 == 0. */
int ifx_vit_unpatch_conv(const ifx_bf16* x, int32_t ldx, int32_t tile_rows, int32_t cls_tokens, const ifx_bf16* weight,
                         const ifx_bf16* bias, ifx_bf16* y, int32_t batch, int32_t t_out, int32_t h_out, int32_t w_out, int32_t patch_t,
                         int32_t patch_h, int32_t patch_w, int32_t channels, void* stream);
/* `TileProcessor.tiled_decode` (inferix/distributed/parallelism/tile_parallel.py:412-448) behind the tile decodes, one pass over the
 * output: blend of every tile with its RAW temporal, upper and left neighbour (in that order), crop to the limits, concatenation, and
 * on request the uint8 tail of `VaeHelper.decode` (inferix/pipeline/magi/video_process.py:195-199).
 *   arena   bf16: the raw decoder outputs; tile (it, ih, iw) is [batch, 3, P_it, H_ih, W_iw], contiguous, at element offset
 *           table[(it tiles_h + ih) tiles_w + iw]; of its P_it >= T_it stored frames the first T_it are the tile (`ViTVAE.decode` keeps
 *           one frame of a single-latent-frame tile, the decoder writes patch_t)
 *   table   int64, in DEVICE memory, read by the kernel only:
 *             [tiles_t tiles_h tiles_w]  arena element offsets, temporal index slowest, width index fastest
 *             then for the axes t, h, w in turn:  [tiles_a] decoded extent of tile k in pixels,  [tiles_a] output start of tile k
 *                                                 (ascending from 0: the sum of min(extent, limit) of its predecessors)
 *             then [tiles_t] frame pitch P of the tiles with temporal index k
 *             then for the axes t, h, w in turn:  [tiles_a][blend_a] blend weights of tile k at position p < e' (see below), one word
 *                                                 per position: the fp32 bits of w1 in the low half, of w2 in the high half
 *   out     bf16 [batch, 3, t_out, h_out, w_out] or NULL;  out_u8  uint8 [batch t_out, 3, h_out, w_out] or NULL; one is required
 * Per output pixel: the owning tile k on an axis is the last one with start <= coordinate, p = coordinate - start.  A blend on an
 * axis is active when k > 0 and p < e' = min(extent[k - 1], extent[k], blend_a); it reads the neighbour at extent[k - 1] - e' + p and
 * computes b = bf16(bf16(a w1) + bf16(b w2)) with the table's weights; the contract for them is w1 = fp32(1.0 - p / e') and
 * w2 = fp32(p / e') with the quotient and the difference in double (the reference's eager bf16 tensor ops with Python-float weights;
 * `1.0f - p / e'` in fp32 differs for extents that are no powers of two; a compiled blend may round once, that form is not built).
 * uint8: trunc(clamp(bf16(bf16(x 127.5) + 127.5), 0, 255)).
 * Checked here: pointers, tiles_a >= 1, limit_a >= 1, 0 <= blend_a <= limit_a, tiles_a <= a_out <= tiles_a limit_a, t_out and
 * 3 batch <= 65535 (grid axes).  The table's
 * contents cannot be checked from the host: the caller guarantees that every read it describes lies inside the arena.
 * vec_x != 0 selects the 16-byte path (one lane per 8 pixels of a row) and promises that every x extent, x start and arena offset in
 * the table is a multiple of 8; it needs w_out, blend_w and (with tiles_w > 1) limit_w % 8 == 0, arena and out 16-byte and out_u8
 * 8-byte aligned.  vec_x == 0 is the one-pixel-per-lane path for any geometry.  No allocation, no synchronisation. */
int ifx_vit_tile_blend(const ifx_bf16* arena, const int64_t* table, ifx_bf16* out, uint8_t* out_u8, int32_t batch, int32_t t_out,
                       int32_t h_out, int32_t w_out, int32_t tiles_t, int32_t tiles_h, int32_t tiles_w, int32_t blend_t, int32_t blend_h,
                       int32_t blend_w, int32_t limit_t, int32_t limit_h, int32_t limit_w, int32_t vec_x, void* stream);
/* The same pass with the uint8 frames written channel-last, the layout a frame consumer takes (`av.VideoFrame.from_ndarray(frame,
 * 'rgb24')`): out_hwc uint8 [batch, t_out, h_out, w_out, 3], bit for bit out_u8 of ifx_vit_tile_blend viewed [batch, t_out, 3, h_out,
 * w_out] and permuted (0, 1, 3, 4, 2).  arena, table, the tile / blend / limit / vec_x arguments and the element arithmetic are those
 * of ifx_vit_tile_blend; one lane owns V pixels of a row and all three channels of them (the batch index is the grid's third axis),
 * vec_x != 0 writes 24 contiguous bytes per lane as three 8-byte stores, vec_x == 0 three bytes.  Checked as there, except: out_hwc
 * must not be NULL, the vec_x path needs arena 16-byte and out_hwc 8-byte aligned, and t_out and batch must each be <= 65535.  No
 * allocation, no synchronisation.  (New export, no struct or signature changes: no ABI bump.) */
int ifx_vit_tile_blend_hwc(const ifx_bf16* arena, const int64_t* table, uint8_t* out_hwc, int32_t batch, int32_t t_out, int32_t h_out,
                           int32_t w_out, int32_t tiles_t, int32_t tiles_h, int32_t tiles_w, int32_t blend_t, int32_t blend_h,
                           int32_t blend_w, int32_t limit_t, int32_t limit_h, int32_t limit_w, int32_t vec_x, void* stream);

/* ----------------------------------------------------------------------
 * MAGI ViT-VAE encoder (the prefix-video encode of image-to-video and video continuation): what `ViTEncoder`
 * (inferix/models/magi/vae/vae_module.py:409-558) and `TileProcessor.tiled_encode` (inferix/distributed/parallelism/tile_parallel.py:
 * 254-346) need besides ifx_layernorm, ifx_gemm_bf16 and the block kernels above.  (New exports, no struct or signature changes: no
 * ABI bump.)
 *
 * Patchify: the A operand of `PatchEmbed.proj` = Conv3d(3 -> D, kernel = stride = patch) as a GEMM with K = 3 patch_t patch_h patch_w,
 * K order (c, t, h, w) = the order of weight.flatten(1).
 *   video    bf16 (is_uint8 == 0) or uint8 pixels; element (n, c, t, h, w) at video + the sum of index x strides[axis]
 *   strides  HOST int64 [5], in elements, >= 0 (0 is the expand of one frame);  dims  HOST int64 [5] = [N, 3, T, H, W]
 *   tiles    HOST int64 [n_tiles][6]: origin (t, h, w) and extent (t, h, w) of every tile in pixels; read and checked here, the
 *            origins travel in the kernel arguments (64 tiles per launch)
 *   rows     bf16 [n_tiles * N * (cls_tokens + lat_t lat_h lat_w), K], row stride ld; tile-major, then sample, then token (t, h, w); the
 *            first cls_tokens rows of every (tile, sample) are left untouched
 * Every tile must lie inside the video and give the launch's latent shape: floor(extent / patch) == lat on every axis, as a strided
 * convolution gives (trailing pixels are never read); an extent smaller than one patch is IFX_EINVAL.  bf16 pixels are copied, uint8
 * pixels become bf16(fp32(v) / 127.5f - 1.0f) (`VaeHelper.encode`'s (video / 127.5) - 1.0, then .bfloat16()).  With patch_w == 8, a
 * unit w stride and 16-byte (uint8: 8-byte) aligned base, strides and origins a lane moves 8 pixels; otherwise one. */
int ifx_vit_patch_rows(const void* video, int32_t is_uint8, const int64_t* strides, const int64_t* dims, const int64_t* tiles,
                       int32_t n_tiles, ifx_bf16* rows, int32_t ld, int32_t cls_tokens, int32_t patch_t, int32_t patch_h,
                       int32_t patch_w, int32_t lat_t, int32_t lat_h, int32_t lat_w, void* stream);
/* `ViTEncoder.forward` :542-557 on token rows x [batch * rows_per_tile, dim] (row stride ldx): affine LayerNorm (fp32 statistics, result
 * rounded to bf16), `last_layer` bf16(fp32 dot + bias) for each of `channels` outputs (weight [channels, dim], bias [channels]), with
 * norm_code the fp32 quotient by the L2 norm over the channels of that token (one rounding).  The first cls_tokens rows of a tile are
 * skipped.  Stored channel-first: channel c < store_channels of token k of tile b at out[b out_batch_stride + c tokens + k], tokens =
 * rows_per_tile - cls_tokens, i.e. [batch, store_channels, lT, lH, lW] when out_batch_stride = store_channels x tokens (store_channels
 * < channels keeps the leading channels: the mean half of the moments).  Built for dim % 8 == 0, dim <= 1024, channels <= 32:
 * anything else is IFX_EUNSUP.  x, gamma, beta, weight 16-byte aligned, ldx % 8 == 0. */
int ifx_vit_latent_head(const ifx_bf16* x, int32_t ldx, const ifx_bf16* gamma, const ifx_bf16* beta, const ifx_bf16* weight,
                        const ifx_bf16* bias, ifx_bf16* out, int64_t out_batch_stride, int32_t batch, int32_t rows_per_tile,
                        int32_t cls_tokens, int32_t dim, int32_t channels, int32_t store_channels, int32_t norm_code, float eps,
                        void* stream);
/* The blend chain of `TileProcessor.tiled_encode` (:312-329), IN PLACE on the encoded tiles as the reference runs it: tile (f, i, j),
 * taken with the temporal index slowest and the width index fastest, is blended on its first e' positions along t with the CURRENT
 * contents of (f - 1, i, j), then along h with (f, i - 1, j), then along w with (f, i, j - 1); e' = min(extent a, extent b, blend).
 * Each blend is b = bf16(bf16(a w1) + bf16(b w2)), a read at extent_a - e' + p, with the table's weights (contract: w1 = fp32(1.0 - p / e'),
 * w2 = fp32(p / e'), quotient and difference in double).  One launch per anti-diagonal f + i + j.
 *   arena   bf16, arena_elements long; tile (f, i, j) is [planes, T_f, H_i, W_j] contiguous at element offset table[(f tiles_h + i) tiles_w + j]
 *   table   int64 in DEVICE memory: [tiles] offsets; [tiles_t] [tiles_h] [tiles_w] extents in latents; for t, h, w in turn
 *           [tiles_a][blend_a] weight words (fp32 bits of w1 low, w2 high); [tiles] tile numbers ordered by diagonal, then ascending
 *   max_tile_elements  HOST int64 [tiles_t + tiles_h + tiles_w - 2]: per diagonal the largest planes x T x H x W of its tiles
 * The kernel checks every address it forms against arena_elements and skips what lies outside.  Crop and concatenation are the
 * caller's.  No allocation, no synchronisation, no device-side wait, no atomic. */
int ifx_vit_latent_blend(ifx_bf16* arena, int64_t arena_elements, const int64_t* table, const int64_t* max_tile_elements, int32_t planes,
                         int32_t tiles_t, int32_t tiles_h, int32_t tiles_w, int32_t blend_t, int32_t blend_h, int32_t blend_w,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INFERIX_HIP_H */

// The row kernels' shared arithmetic and launch plumbing (ifx_norm.hip, ifx_quant.hip, ifx_magi.hip; gfx950): ONE copy of
//   * the register row: branch-free 16-byte chunk loads, fp32 conversion, the two-pass LayerNorm statistics;
//   * the 8-bit packing and the two quantisers (dynamic per-token, static div_clamp_to) of a row held in registers;
//   * the 3-axis RoPE: token -> positions and (cos, sin) pairs, and RMSNorm x weight -> rotation -> bf16 store of one row;
//   * host side: the NCH ladder, the one-wave-per-row launch, the FP8 / INT8 switch, LayerNorm-mode, rope-grid and writer-view
//     validation.
// The fused producers are tested bit for bit against the separate passes (tests/test_hip_quant.py, tests/test_hip_magi_block.py,
// the sequence-parallel rollouts): they now agree because they are the same code, so a slip HERE moves both sides of those tests
// together.  What pins this arithmetic is tests/test_hip_row_kernels.py: every rung and gap of the three NCH ladders, ragged tails,
// row strides, RoPE beyond chunk 0 and offset rows against the CPU oracles.  Rounding points: include/inferix_hip.h.
#pragma once
#include <type_traits>

#include "ifx_common.h"

namespace ifx {

// 16-byte chunks of a row, requested WITHOUT a per-lane branch: a lane whose columns lie beyond `dim` reads the row's first chunk
// instead (a valid address) and its values are zeroed at the conversion.  With the load inside `if (col < dim)` hipcc gave every chunk
// its own basic block — load, s_waitcnt vmcnt(0), convert — so a wave had ONE 1 KiB request in flight at a time and paid the memory
// latency once per chunk (round 4: layernorm 3.1 TB/s, rmsnorm + RoPE + append 3.6 TB/s with three-chunk rows).
template <int NCH>
__device__ __forceinline__ void load_chunks(u16x8 (&u)[NCH], const unsigned short* p, int dim, int lane) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    u[c] = *reinterpret_cast<const u16x8*>(p + (col < dim ? col : 0));
  }
}

template <int NCH>
struct Row {
  float v[NCH][8];
  __device__ __forceinline__ void from(const u16x8 (&u)[NCH], int dim, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const bool ok = c * 512 + lane * 8 < dim;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[c][i] = ok ? bf2f(u[c][i]) : 0.f;
    }
  }
  __device__ __forceinline__ float sum() const {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[c][i];
    return s;
  }
  __device__ __forceinline__ float sumsq() const {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[c][i] * v[c][i];
    return s;
  }
};

// two-pass LayerNorm statistics of a row (lanes beyond `dim` hold zeros and are left out of the squared deviations)
template <int NCH>
__device__ __forceinline__ void ln_stats(const Row<NCH>& row, int dim, float eps, int lane, float& mean, float& rstd) {
  const float inv_n = 1.0f / (float)dim;
  mean = wave_sum(row.sum()) * inv_n;
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c * 512 + lane * 8 < dim) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = row.v[c][i] - mean;
        ss += d * d;
      }
    }
  }
  rstd = 1.0f / sqrtf(wave_sum(ss) * inv_n + eps);
}

// ---------------------------------------------------------------------------
// eight clamped quotients -> eight e4m3 bytes (round-to-nearest-even, v_cvt_pk_fp8_f32) or eight int8 bytes (rint)
template <bool FP8>
__device__ __forceinline__ u32x2 pack8(const float (&v)[8]) {
  if (FP8) {
    unsigned w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], w1, true);
    return u32x2{w0, w1};
  }
  unsigned w[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i >> 2] |= ((unsigned)(int)rintf(v[i]) & 0xffu) << (8 * (i & 3));
  return u32x2{w[0], w[1]};
}

// The dynamic per-token quantiser (scheme: ifx_quant.hip) of a bf16 row in registers, lanes beyond `dim` zeroed by the caller:
// amax -> scale (stored by lane 0) -> bytes at qr[0, dim).
template <bool FP8, int NCH>
__device__ __forceinline__ void quant_row_dynamic(const u16x8 (&u)[NCH], unsigned char* qr, float* scale, int dim, int lane) {
  constexpr float QMAX = FP8 ? 448.0f : 127.0f;
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(u[c][i])));
  amax = wave_max(amax);
  const float s = amax > 0.f ? amax / QMAX : 1.0f;
  if (lane == 0) *scale = s;
  const RowDivisor rdiv(s);        // the exact three-operation x / s (ifx_common.h); 8960-wide rows: 140 quotients per lane
  auto emit = [&](auto fastc) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = c * 512 + lane * 8;
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = fminf(fmaxf(rdiv.template div<decltype(fastc)::value>(bf2f(u[c][i])), -QMAX), QMAX);
      const u32x2 pk = pack8<FP8>(v);
      if (col < dim) *reinterpret_cast<u32x2*>(qr + col) = pk;
    }
  };
  if (rdiv.fast()) emit(std::true_type{});      // ONE wave-uniform branch around the loops
  else emit(std::false_type{});
}

// The static quantiser, div_clamp_to (dit_module.py:367-387), of eight values with their eight divisors: divide, clamp, optionally
// round to bf16 before the cast (dit_module.py:379-384), pack.
template <bool FP8>
__device__ __forceinline__ u32x2 div_clamp8(const float (&x)[8], const f32x4 d0, const f32x4 d1, int via_bf16) {
  constexpr float QMAX = FP8 ? 448.0f : 127.0f;
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float t = fminf(fmaxf(x[i] / (i < 4 ? d0[i] : d1[i - 4]), -QMAX), QMAX);
    v[i] = via_bf16 ? rbf(t) : t;
  }
  return pack8<FP8>(v);
}

// ---------------------------------------------------------------------------
struct RopeArgs {
  const double* freqs;
  int max_pos, start_frame, height, width, hw_offset, hw_local;
  float q_scale = 1.0f;   // applied to the rotated q in fp32 before its ONE rounding to bf16 (ifx_rope_grid.q_scale)
};

// rotate the 4 adjacent-channel pairs held in t[0..7]; pair index jp0..jp0+3 within the head
__device__ __forceinline__ void rope4(float (&t)[8], int jp0, const RopeArgs& ra, int half, int n_t,
                                      int n_h, int pos_t, int pos_h, int pos_w) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int j = jp0 + p;
    const int pos = (j < n_t) ? pos_t : ((j < n_t + n_h) ? pos_h : pos_w);
    const double2 cs = *reinterpret_cast<const double2*>(ra.freqs + ((size_t)pos * half + j) * 2);
    const double a = (double)t[2 * p], b = (double)t[2 * p + 1];
    // complex multiply exactly as (a+ib)(c+is) evaluates in complex128:
    // re = a*c - b*s ; im = a*s + b*c  (each product and sum rounded in fp64)
    const double re = __dmul_rn(a, cs.x) - __dmul_rn(b, cs.y);
    const double im = __dmul_rn(a, cs.y) + __dmul_rn(b, cs.x);
    t[2 * p] = (float)re;       // torch's double->bf16 goes through float
    t[2 * p + 1] = (float)im;
  }
}

// rotation with the four (cos, sin) pairs of this lane already in registers: a lane's 8 channels sit at the same
// offset inside their head in every 512-channel chunk (512 % head_dim == 0), and q and k use the same positions, so
// one set of table reads serves the whole token (was re-read per chunk and per q / k: 24 loads instead of 4)
__device__ __forceinline__ void rope4_cs(float (&t)[8], const double2 (&cs)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double a = (double)t[2 * p], b = (double)t[2 * p + 1];
    const double re = __dmul_rn(a, cs[p].x) - __dmul_rn(b, cs[p].y);
    const double im = __dmul_rn(a, cs[p].y) + __dmul_rn(b, cs[p].x);
    t[2 * p] = (float)re;
    t[2 * p + 1] = (float)im;
  }
}

// Where local row `r` of a launch sits on the (t, h, w) grid, the head's split into the three axes, and — when the shared-pairs form
// applies — this lane's four (cos, sin) pairs, requested here so that they are in flight with the row's own loads.
struct RopeToken {
  int pos_t = 0, pos_h = 0, pos_w = 0;
  int half, n_t, n_h;
  bool shared_cs;
  double2 cs4[4];
  __device__ __forceinline__ RopeToken(const RopeArgs& ra, int has_rope, int r, int head_dim, int lane)
      : half(head_dim >> 1), n_t(half - 2 * (half / 3)), n_h(half / 3), shared_cs(has_rope && (512 % head_dim) == 0) {
    if (has_rope) {
      const int f = r / ra.hw_local;
      const int p = ra.hw_offset + (r - f * ra.hw_local);
      pos_t = ra.start_frame + f;
      pos_h = p / ra.width;
      pos_w = p - pos_h * ra.width;
    }
    if (shared_cs) {
      const int jp0 = ((lane * 8) % head_dim) >> 1;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int j = jp0 + p;
        const int pos = (j < n_t) ? pos_t : ((j < n_t + n_h) ? pos_h : pos_w);
        cs4[p] = *reinterpret_cast<const double2*>(ra.freqs + ((size_t)pos * half + j) * 2);
      }
    }
  }
};

// One q or k row: RMS scale -> bf16 -> x weight -> bf16 -> rotation -> x out_scale -> bf16, handed to put(c, col, chunk) for the
// chunks inside `dim`.  The general rope4 form serves head sizes that do not divide 512 (any head_dim % 16 == 0 through the C ABI).
// `row` is the caller's register row: the append kernel converts q and then k through ONE — with a row of its own per call hipcc put
// that kernel's k-weight loads behind a wait for the V chunks (16 of its 19 loads in flight, profiles/r10_row_kernels_refactor.md).
template <int NCH, typename Put>
__device__ __forceinline__ void rmsnorm_rope_row(Row<NCH>& row, const u16x8 (&raw)[NCH], const u16x8 (&wv)[NCH], const RopeToken& tk,
                                                 const RopeArgs& ra, int has_rope, float out_scale, int dim, int head_dim, float eps,
                                                 int lane, Put&& put) {
  row.from(raw, dim, lane);
  const float rs = 1.0f / sqrtf(wave_sum(row.sumsq()) / (float)dim + eps);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = rbf(rbf(row.v[c][i] * rs) * bf2f(wv[c][i]));
    if (tk.shared_cs) rope4_cs(t, tk.cs4);
    else if (has_rope && col < dim) rope4(t, (col % head_dim) >> 1, ra, tk.half, tk.n_t, tk.n_h, tk.pos_t, tk.pos_h, tk.pos_w);
    u16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2bf(t[i] * out_scale);
    if (col < dim) put(c, col, o);
  }
}

// host side -----------------------------------------------------------------
// f(std::integral_constant<int, N>) for the first N of the caller's ascending list of built row widths, NCH = ceil(dim / 512) chunks,
// that holds the row.  A trailing 0 stands for the caller's generic kernel and takes any width (`too_wide` is then never reached).
// Wider rows than the last N: IFX_EUNSUP with the caller's text, a printf format that takes `dim`.
template <int N, int... WIDER, typename F>
static int dispatch_nch(int dim, const char* too_wide, F&& f) {
  if (N == 0 || (dim + 511) / 512 <= N) return f(std::integral_constant<int, N>{});
  if constexpr (sizeof...(WIDER) > 0) return dispatch_nch<WIDER...>(dim, too_wide, f);
  set_error(too_wide, dim);
  return IFX_EUNSUP;
}

// one wavefront per row, four per workgroup
template <typename K, typename... A>
static int launch_rows(const char* who, K kernel, int rows, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, args...);
  return check_launch(who);
}

// f(std::true_type) for IFX_Q_FP8_E4M3, f(std::false_type) for IFX_Q_INT8 (the caller has validated `format`)
template <typename F>
static int dispatch_q8_format(int format, F&& f) {
  return format == IFX_Q_FP8_E4M3 ? f(std::true_type{}) : f(std::false_type{});
}

static int check_ln_mode(const char* who, int mode, const void* gamma, const void* beta, const void* mod, int mod_slots,
                         int shift_slot, int scale_slot, int rows_per_group) {
  IFX_REQUIRE(mode >= IFX_LN_PLAIN && mode <= IFX_LN_MODULATE, "%s: bad mode %d", who, mode);
  if (mode == IFX_LN_AFFINE) IFX_REQUIRE(gamma && beta, "%s: affine mode needs gamma/beta", who);
  if (mode == IFX_LN_MODULATE)
    IFX_REQUIRE(mod && rows_per_group > 0 && mod_slots > 0 && shift_slot >= 0 && shift_slot < mod_slots &&
                    scale_slot >= 0 && scale_slot < mod_slots,
                "%s: modulate mode needs mod/slots/rows_per_group", who);
  return IFX_OK;
}

// ifx_rope_grid -> RopeArgs for `rows` local tokens (nullptr: no rotation, *ra stays as it is); q_scale and flags are the caller's
static int resolve_rope(const char* who, const ifx_rope_grid* rope, int head_dim, int dim, int rows, RopeArgs* ra) {
  if (rope == nullptr) return IFX_OK;
  IFX_REQUIRE(rope->freqs && rope->hw_local > 0 && rope->width > 0 && rope->height > 0, "%s: bad rope grid", who);
  IFX_REQUIRE(head_dim % 16 == 0 && dim % head_dim == 0, "%s: head_dim %d", who, head_dim);
  // the rows' hw indices [hw_offset, hw_offset + hw_local) lie on the height x width grid: pos_h = hw / width indexes the table
  IFX_REQUIRE(rope->hw_offset >= 0 && (long long)rope->hw_offset + rope->hw_local <= (long long)rope->height * rope->width,
              "%s: rope hw_offset %d + hw_local %d outside the %d x %d grid", who, rope->hw_offset, rope->hw_local, rope->height,
              rope->width);
  const int frames = (rows + rope->hw_local - 1) / rope->hw_local;
  IFX_REQUIRE(rope->start_frame + frames <= rope->max_pos && rope->height <= rope->max_pos && rope->width <= rope->max_pos,
              "%s: positions exceed rope table (%d)", who, rope->max_pos);
  *ra = RopeArgs{rope->freqs, rope->max_pos, rope->start_frame, rope->height, rope->width, rope->hw_offset, rope->hw_local};
  return IFX_OK;
}

// The kernels that WRITE cache rows by logical token (append, roll, scatter) address them through the page table or the identity map.
// The two-segment map of ifx_kv_view is for readers (and ifx_rmsnorm_rope_kv_push, which honours it): no caller hands such a view
// to a writer — MAGI, the only producer of segment views, stores its rows with ifx_magi_head_prep / ifx_kv_split_rows — so a
// writer refuses it instead of storing to the unmapped slot.
static int check_writer_view(const char* who, const ifx_kv_view* kv) {
  if (kv->page_table) IFX_REQUIRE(kv->page_size > 0, "%s: page_size must be > 0", who);
  else IFX_REQUIRE(kv->seg_split <= 0, "%s: kv view with a two-segment map (seg_split %d) and no page table: the map is for readers",
                   who, kv->seg_split);
  return IFX_OK;
}

}  // namespace ifx

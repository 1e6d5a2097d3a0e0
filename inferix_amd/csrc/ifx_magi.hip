// Row kernels of the MAGI transformer layer (BASELINE config 5; gfx950).  All HBM-bound: one pass over the row, 16-byte accesses,
// statistics by wavefront shuffles, every elementwise neighbour fused in.
//
//   magi_head_prep_kernel   : what FullyParallelAttention.get_q / get_k / get_v / get_xqkv do between the projections and the
//                             attention calls (inferix/models/magi/dit/dit_module.py:902-970): per-HEAD LayerNorm over 128 channels
//                             (fp32 module + rotary for q / k, bf16 module for the cross-attention query / key), non-interleaved
//                             rotary embedding, and the scatter of k / v rows to where attention reads them (the in-place cache,
//                             or the staging buffer of the Ulysses all-to-all).  One 16-lane group per head, four heads per wave.
//   magi_gate_norm_kernel   : bias_modulate_add (dit_module.py:295-313) = the Triton range_mod kernel (:204-292) + post-norm +
//                             residual: y = bf16( LN_fp32( float(x) * float(gate[map[row]]) ) + float(residual) ).  The gate cannot
//                             ride in the producing GEMM's epilogue here: the LayerNorm that follows it needs the statistics of
//                             the whole 3072-wide row, a GEMM tile sees 128-256 columns of it.
//   act_rows_kernel         : SiLU / softcap(tanh) of AdaModulateLayer + gating_and_mlp (:196-198,:363-364,:1300-1303).
//   silu_and_mul_kernel     : the gated MLP's activation (flashinfer silu_and_mul, :548-549; the 24B configs), bf16 and / or the e4m3
//                             bytes of the FP8 fc2's input.
//   quant_static_kernel     : the static-scale / per-tensor quantisers (div_clamp_to).
// The register row, the LayerNorm statistics, div_clamp8 and the launch helpers are those of ifx_rows.h (shared with ifx_norm.hip and
// ifx_quant.hip); magi_head_prep_kernel works on 16-lane head groups and keeps its own arithmetic.
#include "ifx_rows.h"

namespace ifx {

// head types of magi_head_prep_kernel
enum { HT_Q = 0, HT_QX = 1, HT_K = 2, HT_V = 3, HT_KX = 4 };

struct HeadPrepArgs {
  const unsigned short* in;      // [rows, ld_in]
  int ld_in, rows, n_heads;      // n_heads 128-wide head slots per row
  int layout;                    // 0: [HQ q | HQ qx | HK k | HK v]      1: HK x (kx | v) interleaved (linear_kv_xattn output)
  int hq, hk;
  const float* rope;             // [rows, 2 * rope_half] fp32 = (sin | cos) per token (rotary_pos_emb, dit_module.py:1097)
  int rope_half;                 // rotary pairs per head: channel e < rope_half pairs with e + rope_half, channels >= 2 rope_half pass
  const float* qn_w;             // fp32 [128] q_layernorm / k_layernorm (high-precision modules, dit_model.py:620-637)
  const float* qn_b;
  const float* kn_w;
  const float* kn_b;
  const unsigned short* xn_w;    // bf16 [128] q_layernorm_xattn (layout 0) or k_layernorm_xattn (layout 1)
  const unsigned short* xn_b;
  float eps;
  int one_p;                     // apply_layernorm_1p: weight + 1 (in the parameter's dtype)
  unsigned short* q_out;         // [rows, ld_q]   head h at column h * 128
  int ld_q;
  unsigned short* qx_out;        // [rows, ld_qx]
  int ld_qx;
  unsigned short* k_out;         // k / v rows: row r goes to dest(r) * ld_kv + head * kv_head_stride
  unsigned short* v_out;
  int ld_kv, kv_head_stride;
  int row0, split, row1;         // dest(r) = r < split ? row0 + r : row1 + (r - split)
  float q_scale;                 // self-attention q only: applied in fp32 before the rounding to bf16 (1 = the reference's q)
  int q_group;                   // 0: head h of q at column h * 128 of row r; > 0: at (h / q_group) * q_group_stride + r * ld_q + (h % q_group) * 128
  long long q_group_stride;      //    (the head -> rank all-to-all's send order)
};

__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

__global__ __launch_bounds__(256) void magi_head_prep_kernel(HeadPrepArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int chunks = (A.n_heads + 3) >> 2;                 // four heads (512 channels) per wave
  const int r = wave / chunks, chunk = wave - r * chunks;
  if (r >= A.rows) return;
  const int head = chunk * 4 + (lane >> 4);
  if (head >= A.n_heads) return;
  const int e0 = (lane & 15) * 8;                          // this lane's 8 channels inside the head
  int type, hidx;
  if (A.layout == 0) {
    if (head < A.hq) type = HT_Q, hidx = head;
    else if (head < 2 * A.hq) type = HT_QX, hidx = head - A.hq;
    else if (head < 2 * A.hq + A.hk) type = HT_K, hidx = head - 2 * A.hq;
    else type = HT_V, hidx = head - 2 * A.hq - A.hk;
  } else {
    type = (head & 1) ? HT_V : HT_KX;
    hidx = head >> 1;
  }
  const u16x8 u = *reinterpret_cast<const u16x8*>(A.in + (size_t)r * A.ld_in + head * 128 + e0);
  const int dest = r < A.split ? A.row0 + r : A.row1 + (r - A.split);
  if (type == HT_V) {                                      // get_v: a copy into the cache / staging layout
    *reinterpret_cast<u16x8*>(A.v_out + (size_t)dest * A.ld_kv + hidx * A.kv_head_stride + e0) = u;
    return;
  }
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = bf2f(u[i]);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += v[i];
  const float mean = group16_sum(s) * (1.0f / 128.0f);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float d = v[i] - mean;
    ss += d * d;
  }
  const float rstd = 1.0f / sqrtf(group16_sum(ss) * (1.0f / 128.0f) + A.eps);
  u16x8 o;
  if (type == HT_QX || type == HT_KX) {
    // FusedLayerNorm as a bf16 module on a bf16 tensor: weight + 1 evaluated in bf16, fp32 math inside, one rounding
    const u16x8 w = *reinterpret_cast<const u16x8*>(A.xn_w + e0);
    const u16x8 b = *reinterpret_cast<const u16x8*>(A.xn_b + e0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float wi = A.one_p ? rbf(bf2f(w[i]) + 1.0f) : bf2f(w[i]);
      o[i] = f2bf((v[i] - mean) * rstd * wi + bf2f(b[i]));
    }
    if (type == HT_QX) *reinterpret_cast<u16x8*>(A.qx_out + (size_t)r * A.ld_qx + hidx * 128 + e0) = o;
    else *reinterpret_cast<u16x8*>(A.k_out + (size_t)dest * A.ld_kv + hidx * A.kv_head_stride + e0) = o;
    return;
  }
  // q / k: fp32 LayerNorm (weights fp32), then the non-interleaved rotary in fp32, one rounding to bf16
  const float* wp = type == HT_Q ? A.qn_w : A.kn_w;
  const float* bp = type == HT_Q ? A.qn_b : A.kn_b;
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + e0), w1 = *reinterpret_cast<const f32x4*>(wp + e0 + 4);
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp + e0), b1 = *reinterpret_cast<const f32x4*>(bp + e0 + 4);
  const float one = A.one_p ? 1.0f : 0.0f;
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float wi = (i < 4 ? w0[i] : w1[i - 4]) + one;
    const float bi = i < 4 ? b0[i] : b1[i - 4];
    y[i] = (v[i] - mean) * rstd * wi + bi;
  }
  // rotary over the first 2 * rope_half channels of the head (flash-attn's non-interleaved form: x1 = [0, half), x2 = [half, 2 half);
  // MAGI's table has 3 axes x head_dim / 8 bands = 96 of 128 channels, dit_module.py:673-720): channel e pairs with e +- half = the
  // lane half / 8 further inside this 16-lane head group; the channels behind the rotary width pass through
  const int half = A.rope_half;
  const bool rot = e0 < 2 * half, lo = e0 < half;
  const int j0 = rot ? (lo ? e0 : e0 - half) : 0;          // index into sin / cos
  const float* rp = A.rope + (size_t)r * (2 * half);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(rp + j0), s1 = *reinterpret_cast<const f32x4*>(rp + j0 + 4);
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(rp + half + j0), c1 = *reinterpret_cast<const f32x4*>(rp + half + j0 + 4);
  const int partner = rot ? lane + (lo ? (half >> 3) : -(half >> 3)) : lane;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float p = __shfl(y[i], partner, 64);
    const float sn = i < 4 ? s0[i] : s1[i - 4], cs = i < 4 ? c0[i] : c1[i - 4];
    // out1 = x1 * cos - x2 * sin ; out2 = x1 * sin + x2 * cos   (products rounded separately, as the elementwise torch ops do)
    const float out = !rot ? y[i] : (lo ? __fmul_rn(y[i], cs) - __fmul_rn(p, sn) : __fmul_rn(p, sn) + __fmul_rn(y[i], cs));
    o[i] = f2bf(type == HT_Q ? out * A.q_scale : out);
  }
  if (type == HT_Q) {
    const size_t qcol = A.q_group > 0 ? (size_t)(hidx / A.q_group) * (size_t)A.q_group_stride + (size_t)(hidx % A.q_group) * 128
                                      : (size_t)hidx * 128;
    *reinterpret_cast<u16x8*>(A.q_out + (size_t)r * A.ld_q + qcol + e0) = o;
  } else {
    *reinterpret_cast<u16x8*>(A.k_out + (size_t)dest * A.ld_kv + hidx * A.kv_head_stride + e0) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void magi_gate_norm_kernel(const unsigned short* __restrict__ x, int ldx,
                                                             const unsigned short* __restrict__ residual, int ldr,
                                                             const int32_t* __restrict__ map,
                                                             const unsigned short* __restrict__ gate, int ld_gate,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             int one_p, unsigned short* __restrict__ y, int ldy, int rows,
                                                             int dim, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const unsigned short* xr = x + (size_t)r * ldx;
  const unsigned short* rr = residual + (size_t)r * ldr;
  const unsigned short* gr = gate + (size_t)map[r] * ld_gate;
  // every request of the row up front and branch-free (x, gate, residual and the fp32 norm weights, which do not depend on the
  // statistics): with the loads inside `if (col < dim)` hipcc waited for each 512-channel chunk before requesting the next — six
  // memory latencies per 3072-wide row (round 4; the load_chunks of ifx_rows.h)
  u16x8 xu[NCH], gu[NCH], res[NCH];
  f32x4 w0[NCH], w1[NCH], b0[NCH], b1[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {                 // chunk by chunk, not load_chunks per array: that order measured 5 % slower (r10 profile)
    const int col = c * 512 + lane * 8;
    const int cc = col < dim ? col : 0;
    xu[c] = *reinterpret_cast<const u16x8*>(xr + cc);
    gu[c] = *reinterpret_cast<const u16x8*>(gr + cc);
    res[c] = *reinterpret_cast<const u16x8*>(rr + cc);
  }
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    const int cc = col < dim ? col : 0;
    w0[c] = *reinterpret_cast<const f32x4*>(w + cc), w1[c] = *reinterpret_cast<const f32x4*>(w + cc + 4);
    b0[c] = *reinterpret_cast<const f32x4*>(b + cc), b1[c] = *reinterpret_cast<const f32x4*>(b + cc + 4);
  }
  Row<NCH> row;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const bool ok = c * 512 + lane * 8 < dim;
#pragma unroll
    for (int i = 0; i < 8; ++i) row.v[c][i] = ok ? bf2f(xu[c][i]) * bf2f(gu[c][i]) : 0.f;       // range_mod in fp32
  }
  float mean, rstd;
  ln_stats(row, dim, eps, lane, mean, rstd);
  const float one = one_p ? 1.0f : 0.0f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    u16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float wi = (i < 4 ? w0[c][i] : w1[c][i - 4]) + one;
      const float bi = i < 4 ? b0[c][i] : b1[c][i - 4];
      const float n = (row.v[c][i] - mean) * rstd * wi + bi;               // post_norm in fp32
      o[i] = f2bf(n + bf2f(res[c][i]));                                    // + residual.float(), one rounding
    }
    if (col < dim) *reinterpret_cast<u16x8*>(y + (size_t)r * ldy + col) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------
// mode 0: SiLU as torch evaluates it on a bf16 tensor (fp32 x / (1 + exp(-x)), one rounding)
// mode 1: softcap with cap 1: bf16(tanh(float(x)))
__global__ __launch_bounds__(256) void act_rows_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                       long n, int mode) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = bf2f(x[i]);
  y[i] = f2bf(mode == 0 ? v / (1.0f + expf(-v)) : tanhf(v));
}

// ---------------------------------------------------------------------------------------------------------
// The gated MLP's activation (CustomMLP with gated_linear_unit, dit_module.py:528-549: flashinfer.activation.silu_and_mul on the fc1
// output [rows, gate (f) | up (f)]) as the repository's oracle restates it and the reference-generated fixtures pin it
// (oracle/magi_block_oracle.py:300-302):  y = bf16( bf16(silu_fp32(gate)) * up )  — SiLU in fp32 rounded to bf16, then the product
// of the two bf16 values rounded again.  flashinfer's own kernel keeps fp32 between the two steps (ONE rounding); its source is not in
// the reference tree, so that form is unpinned here and the two-rounding chain is what this kernel evaluates.
// Elementwise: one lane per 8-column chunk, 16-byte loads and stores, grid-stride over (row, chunk) with the (row, chunk) pair advanced
// by additions (one division per lane, before the loop).  `q`: the bf16 result through ifx_quant_static's rule (div_clamp8, e4m3) for
// the FP8 fc2, instead of or next to `y`.
__global__ __launch_bounds__(256) void silu_and_mul_kernel(const unsigned short* __restrict__ x, int ldx,
                                                           unsigned short* __restrict__ y, int ldy, unsigned char* __restrict__ q, int ldq,
                                                           const float* __restrict__ divisor, int divisor_is_vector, int rows, int f) {
  const int cpr = f >> 3;                                   // chunks per row
  const int stride = (int)gridDim.x * 256;                  // <= 2048 x 256 lanes (the launcher's cap)
  const int i0 = (int)blockIdx.x * 256 + (int)threadIdx.x;
  long r = i0 / cpr;
  int c = i0 - (int)r * cpr;
  const int dr = stride / cpr, dc = stride - dr * cpr;
  float s1 = 1.0f;
  if (q != nullptr && !divisor_is_vector) s1 = divisor[0];
  for (; r < rows; r += dr) {
    const int col = c * 8;
    const unsigned short* xr = x + (size_t)r * ldx + col;
    const u16x8 g = *reinterpret_cast<const u16x8*>(xr);
    const u16x8 u = *reinterpret_cast<const u16x8*>(xr + f);
    f32x4 d0 = f32x4{s1, s1, s1, s1}, d1 = d0;
    if (q != nullptr && divisor_is_vector) {
      d0 = *reinterpret_cast<const f32x4*>(divisor + col);
      d1 = *reinterpret_cast<const f32x4*>(divisor + col + 4);
    }
    u16x8 o;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float a = bf2f(g[i]);
      // a / (1 + exp(-a)) with exp(-a) = exp2(-a log2 e) and the hardware reciprocal: both within an fp32 ULP or two, far below the
      // bf16 rounding that follows
      const float s = rbf(a * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(a * -1.4426950408889634f)));
      o[i] = f2bf(s * bf2f(u[i]));
      v[i] = bf2f(o[i]);
    }
    if (y != nullptr) *reinterpret_cast<u16x8*>(y + (size_t)r * ldy + col) = o;
    if (q != nullptr) *reinterpret_cast<u32x2*>(q + (size_t)r * ldq + col) = div_clamp8<true>(v, d0, d1, 1);
    c += dc;
    if (c >= cpr) {
      c -= cpr;
      ++r;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Static-scale / per-tensor quantisers (see include/inferix_hip.h, ifx_quant_static / ifx_quant_per_tensor)
__global__ __launch_bounds__(256) void amax_kernel(const unsigned short* __restrict__ x, int ldx, int rows, int K,
                                                   unsigned* __restrict__ amax_bits) {
  float m = 0.f;
  const int chunks_per_row = K / 8;
  const long total = (long)rows * chunks_per_row;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int r = (int)(i / chunks_per_row), c = (int)(i - (long)r * chunks_per_row);
    const u16x8 u = *reinterpret_cast<const u16x8*>(x + (size_t)r * ldx + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(bf2f(u[e])));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax_bits, __builtin_bit_cast(unsigned, m));   // non-negative floats order as uints
}

// SCALE: 0 = divisor vector [K] (per input channel), 1 = one divisor at scale[0], 2 = amax_bits[0] / QMAX (1 when amax == 0)
template <bool FP8>
__global__ __launch_bounds__(256) void quant_static_kernel(const unsigned short* __restrict__ x, int ldx,
                                                           unsigned char* __restrict__ q, int ldq,
                                                           const float* __restrict__ scale, int scale_mode,
                                                           const unsigned* __restrict__ amax_bits, float* __restrict__ row_scale,
                                                           int rows, int K, int via_bf16) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  constexpr float QMAX = FP8 ? 448.0f : 127.0f;
  float s1 = 1.0f;
  if (scale_mode == 1) s1 = scale[0];
  if (scale_mode == 2) {
    const float amax = __builtin_bit_cast(float, amax_bits[0]);
    s1 = amax > 0.f ? amax / QMAX : 1.0f;
  }
  if (row_scale != nullptr && lane == 0 && scale_mode != 0) row_scale[r] = s1;      // a divisor vector has no row scale: left alone
  // four 512-column chunks per pass, every load of the pass (16 B of x, 32 B of divisors per lane and chunk) issued before the first
  // use: one wave per row has nothing else to hide the latency with (56 -> ~20 us on 6075 x 3072)
  constexpr int UN = 4;
  for (int col0 = lane * 8; col0 < K; col0 += 512 * UN) {
    u16x8 u[UN];
    f32x4 d0[UN], d1[UN];
#pragma unroll
    for (int c = 0; c < UN; ++c) {
      const int col = col0 + 512 * c;
      if (col < K) {
        u[c] = *reinterpret_cast<const u16x8*>(x + (size_t)r * ldx + col);
        if (scale_mode == 0) {
          d0[c] = *reinterpret_cast<const f32x4*>(scale + col);
          d1[c] = *reinterpret_cast<const f32x4*>(scale + col + 4);
        } else {
          d0[c] = d1[c] = f32x4{s1, s1, s1, s1};
        }
      }
    }
#pragma unroll
    for (int c = 0; c < UN; ++c) {
      const int col = col0 + 512 * c;
      if (col >= K) continue;
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = bf2f(u[c][i]);
      const u32x2 pk = div_clamp8<FP8>(v, d0[c], d1[c], via_bf16);
      *reinterpret_cast<u32x2*>(q + (size_t)r * ldq + col) = pk;
    }
  }
}

}  // namespace ifx

using namespace ifx;

extern "C" int ifx_magi_head_prep(const ifx_magi_head_prep_desc* d, void* stream) {
  IFX_REQUIRE(d && d->in && d->rows >= 0 && d->ld_in % 8 == 0, "ifx_magi_head_prep: bad input");
  IFX_REQUIRE(d->head_dim == 128, "ifx_magi_head_prep: head_dim %d not built (128 only)", d->head_dim);
  IFX_REQUIRE(d->layout == 0 || d->layout == 1, "ifx_magi_head_prep: layout %d", d->layout);
  HeadPrepArgs a{};
  a.in = d->in;
  a.ld_in = d->ld_in;
  a.rows = d->rows;
  a.layout = d->layout;
  a.hq = d->q_heads;
  a.hk = d->kv_heads;
  IFX_REQUIRE(a.hk > 0, "ifx_magi_head_prep: kv_heads must be > 0");
  if (d->layout == 0) {
    IFX_REQUIRE(a.hq > 0 && d->rope && d->qn_w && d->qn_b && d->kn_w && d->kn_b && d->xn_w && d->xn_b && d->q_out && d->qx_out,
                "ifx_magi_head_prep: layout 0 needs q/qx outputs, rope and the three norms");
    IFX_REQUIRE(d->q_group >= 0 && (d->q_group == 0 || (a.hq % d->q_group == 0 && d->q_group_stride >= (int64_t)d->rows * d->ld_q && d->q_group_stride % 8 == 0)),
                "ifx_magi_head_prep: q_group %d / q_group_stride %lld", d->q_group, (long long)d->q_group_stride);
    IFX_REQUIRE(d->ld_q >= (d->q_group > 0 ? d->q_group : a.hq) * 128 && d->ld_qx >= a.hq * 128 && d->ld_q % 8 == 0 && d->ld_qx % 8 == 0,
                "ifx_magi_head_prep: q row strides too small");
    a.n_heads = 2 * a.hq + 2 * a.hk;
  } else {
    IFX_REQUIRE(d->xn_w && d->xn_b, "ifx_magi_head_prep: layout 1 needs k_layernorm_xattn");
    a.n_heads = 2 * a.hk;
  }
  IFX_REQUIRE(d->ld_in >= a.n_heads * 128, "ifx_magi_head_prep: ld_in %d < %d heads x 128", d->ld_in, a.n_heads);
  IFX_REQUIRE(d->k_out && d->v_out && d->ld_kv % 8 == 0 && d->kv_head_stride % 8 == 0 && d->kv_head_stride >= 128,
              "ifx_magi_head_prep: k/v destination");
  IFX_REQUIRE(d->split >= 0 && d->row0 >= 0 && d->row1 >= 0, "ifx_magi_head_prep: negative destination rows");
  a.rope = d->rope;
  a.rope_half = d->rope_half > 0 ? d->rope_half : 64;
  IFX_REQUIRE(a.rope_half % 8 == 0 && a.rope_half <= 64, "ifx_magi_head_prep: rope_half (%d) must be a multiple of 8, at most 64", a.rope_half);
  a.qn_w = d->qn_w, a.qn_b = d->qn_b, a.kn_w = d->kn_w, a.kn_b = d->kn_b;
  a.xn_w = d->xn_w, a.xn_b = d->xn_b;
  a.eps = d->eps;
  a.one_p = d->layernorm_1p ? 1 : 0;
  a.q_out = d->q_out, a.ld_q = d->ld_q, a.qx_out = d->qx_out, a.ld_qx = d->ld_qx;
  IFX_REQUIRE(d->q_scale >= 0.f && d->q_scale == d->q_scale, "ifx_magi_head_prep: q_scale must be >= 0 (0 = 1)");
  a.q_scale = d->q_scale > 0.f ? d->q_scale : 1.0f;
  a.q_group = d->q_group, a.q_group_stride = d->q_group_stride;
  a.k_out = d->k_out, a.v_out = d->v_out, a.ld_kv = d->ld_kv, a.kv_head_stride = d->kv_head_stride;
  a.row0 = d->row0, a.split = d->split, a.row1 = d->row1;
  if (d->rows == 0) return IFX_OK;
  const long waves = (long)d->rows * ((a.n_heads + 3) / 4);
  hipLaunchKernelGGL(magi_head_prep_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_magi_head_prep");
}

extern "C" int ifx_magi_gate_norm_residual(const ifx_bf16* x, int32_t ldx, const ifx_bf16* residual, int32_t ld_res,
                                           const int32_t* condition_map, const ifx_bf16* gate, int32_t ld_gate,
                                           const float* norm_w, const float* norm_b, int32_t layernorm_1p, ifx_bf16* y,
                                           int32_t ldy, int32_t rows, int32_t dim, float eps, void* stream) {
  IFX_REQUIRE(x && residual && condition_map && gate && norm_w && norm_b && y && rows >= 0 && dim > 0 && dim % 8 == 0,
              "ifx_magi_gate_norm_residual: bad arguments (dim %d)", dim);
  IFX_REQUIRE(ldx % 8 == 0 && ld_res % 8 == 0 && ld_gate % 8 == 0 && ldy % 8 == 0 && ldx >= dim && ld_res >= dim && ldy >= dim,
              "ifx_magi_gate_norm_residual: row strides must be >= dim and multiples of 8");
  if (rows == 0) return IFX_OK;
  return dispatch_nch<1, 2, 4, 6, 8, 12>(dim, "ifx_magi_gate_norm_residual: dim <= 6144 supported (got %d)", [&](auto nch) {
    return launch_rows("ifx_magi_gate_norm_residual", magi_gate_norm_kernel<decltype(nch)::value>, rows, stream, x, ldx, residual, ld_res,
                       condition_map, gate, ld_gate, norm_w, norm_b, layernorm_1p ? 1 : 0, y, ldy, rows, dim, eps);
  });
}

// K | V rows of an all-to-all message -> the cache planes, with the store rule's two destination runs (MagiKVCacheManager): row r of
// `kv` [n, heads, 2 * 128] goes to cache row dest(r) = r < split ? row0 + r : row1 + (r - split); K = the first 128 channels of a head,
// V the second.  One launch for what four strided torch copies did (k / v x stored run / scratch run).
namespace ifx {
__global__ __launch_bounds__(256) void kv_split_rows_kernel(const unsigned short* __restrict__ kv, unsigned short* __restrict__ kc,
                                                            unsigned short* __restrict__ vc, long n_chunks, int heads, int row0,
                                                            int split, int row1) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;          // one 16-byte chunk of K and the matching one of V per thread
  if (c >= n_chunks) return;
  const int ch = (int)(c & 15);                                 // chunk inside the 128-channel head
  const long rh = c >> 4;                                       // (row, head)
  const int h = (int)(rh % heads);
  const long r = rh / heads;
  const long dest = r < split ? (long)row0 + r : (long)row1 + (r - split);
  const u16x8 k = *reinterpret_cast<const u16x8*>(kv + (rh * 2) * 128 + ch * 8);
  const u16x8 v = *reinterpret_cast<const u16x8*>(kv + (rh * 2 + 1) * 128 + ch * 8);
  *reinterpret_cast<u16x8*>(kc + (dest * heads + h) * 128 + ch * 8) = k;
  *reinterpret_cast<u16x8*>(vc + (dest * heads + h) * 128 + ch * 8) = v;
}
}  // namespace ifx

extern "C" int ifx_kv_split_rows(const ifx_bf16* kv, ifx_bf16* k_cache, ifx_bf16* v_cache, int32_t rows, int32_t heads, int32_t row0,
                                 int32_t split, int32_t row1, void* stream) {
  IFX_REQUIRE(kv && k_cache && v_cache && rows >= 0 && heads > 0 && row0 >= 0 && row1 >= 0 && split >= 0 && split <= rows,
              "ifx_kv_split_rows: bad arguments (rows %d, heads %d, split %d)", rows, heads, split);
  IFX_REQUIRE(!((uintptr_t)kv & 15) && !((uintptr_t)k_cache & 15) && !((uintptr_t)v_cache & 15), "ifx_kv_split_rows: 16-byte aligned tensors");
  if (rows == 0) return IFX_OK;
  const long n_chunks = (long)rows * heads * 16;
  hipLaunchKernelGGL(ifx::kv_split_rows_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kv, k_cache,
                     v_cache, n_chunks, heads, row0, split, row1);
  return check_launch("ifx_kv_split_rows");
}

// The glue between two model forwards (SampleTransport.forward_velocity's tail + integrate, video_generate.py:531-552, and the mixes
// of forward_dispatcher, dit_model.py:500-596): x += (w0 v0 [+ w1 v1] [+ w2 v2]) * dt per chunk of the window, every operator rounded on
// its own as the torch sequence rounds it.  HBM-bound (config 5: 12 MB of x and up to 37 MB of velocities per step).  One
// (channel, chunk) span — chunk_width H W contiguous floats in x and in every source — per blockIdx.y, grid-strided along blockIdx.x.
// A span's start is 16-byte aligned only when the element offsets of x and of the sources agree mod 4 (H W odd: they do not): then the
// body moves 16 bytes per lane and the ragged head and tail 4; otherwise the whole span goes 4 bytes at a time.
namespace ifx {
struct IntegrateArgs {
  float* x;
  long row_stride, chan_stride, x_first;       // x_first: element offset of the window inside a channel
  int rows, n_chunks, n_src;
  long span;                                    // chunk_width * H * W
  float dt[IFX_MAGI_INTEGRATE_MAX_CHUNKS];
  const float* v[IFX_MAGI_INTEGRATE_MAX_SOURCES];
  long v_chan_stride[IFX_MAGI_INTEGRATE_MAX_SOURCES];
  long v_first[IFX_MAGI_INTEGRATE_MAX_SOURCES]; // element offset, inside a channel, of what lies under window chunk first_chunk
  int c0[IFX_MAGI_INTEGRATE_MAX_SOURCES], c1[IFX_MAGI_INTEGRATE_MAX_SOURCES];
  float w[IFX_MAGI_INTEGRATE_MAX_SOURCES][IFX_MAGI_INTEGRATE_MAX_CHUNKS];
};

__device__ __forceinline__ float integrate_one(float x, float a, float b, float c, float w0, float w1, float w2, float dt, bool h1,
                                               bool h2) {
  // Every product and sum rounded on its own.  __fmul_rn / __fadd_rn do not hold that here: they are inline `*` and `+` compiled under
  // the default -ffp-contract=fast, and hipcc fuses a sum with the product feeding it across them (v_fma_f32 in the listing).  With
  // contraction switched off for this block the operators carry no `contract` flag and stay v_mul_f32 / v_add_f32 after inlining.
#pragma clang fp contract(off)
  float m = w0 * a;
  if (h1) m = m + w1 * b;
  if (h2) m = m + w2 * c;
  return x + m * dt;
}

__global__ __launch_bounds__(256) void magi_integrate_kernel(IntegrateArgs A) {
  const int ch = blockIdx.y / A.n_chunks, c = blockIdx.y - ch * A.n_chunks;
  float* __restrict__ x0 = A.x + ch * A.chan_stride + A.x_first + c * A.span;
  float* __restrict__ x1 = x0 + A.row_stride;                            // stored only when rows == 2
  const bool two = A.rows == 2;
  const bool h1 = A.n_src > 1 && c >= A.c0[1] && c <= A.c1[1];
  const bool h2 = A.n_src > 2 && c >= A.c0[2] && c <= A.c1[2];
  const float* __restrict__ v0 = A.v[0] + ch * A.v_chan_stride[0] + A.v_first[0] + (c - A.c0[0]) * A.span;
  const float* __restrict__ v1 = h1 ? A.v[1] + ch * A.v_chan_stride[1] + A.v_first[1] + (c - A.c0[1]) * A.span : v0;
  const float* __restrict__ v2 = h2 ? A.v[2] + ch * A.v_chan_stride[2] + A.v_first[2] + (c - A.c0[2]) * A.span : v0;
  const float w0 = A.w[0][c], w1 = A.w[1][c], w2 = A.w[2][c], dt = A.dt[c];
  const unsigned mis = (unsigned)((uintptr_t)x0 & 15);
  const bool vec = ((uintptr_t)v0 & 15) == mis && ((uintptr_t)v1 & 15) == mis && ((uintptr_t)v2 & 15) == mis &&
                   (!two || ((uintptr_t)x1 & 15) == mis);
  long head = vec ? (long)(((16u - mis) & 15u) >> 2) : A.span;           // scalar elements in front of the 16-byte body
  if (head > A.span) head = A.span;
  const long nv = (A.span - head) >> 2;                                   // 16-byte groups of the body
  const long tail0 = head + (nv << 2);                                    // scalar elements behind it: [tail0, span)
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  for (long i = tid; i < nv; i += stride) {
    const long e = head + (i << 2);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x0 + e);
    const f32x4 a = *reinterpret_cast<const f32x4*>(v0 + e);
    f32x4 b = a, cc = a;
    if (h1) b = *reinterpret_cast<const f32x4*>(v1 + e);
    if (h2) cc = *reinterpret_cast<const f32x4*>(v2 + e);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = integrate_one(xv[k], a[k], b[k], cc[k], w0, w1, w2, dt, h1, h2);
    *reinterpret_cast<f32x4*>(x0 + e) = r;
    if (two) *reinterpret_cast<f32x4*>(x1 + e) = r;
  }
  const long n_scalar = head + (A.span - tail0);
  for (long i = tid; i < n_scalar; i += stride) {
    const long e = i < head ? i : tail0 + (i - head);
    const float r = integrate_one(x0[e], v0[e], h1 ? v1[e] : 0.f, h2 ? v2[e] : 0.f, w0, w1, w2, dt, h1, h2);
    x0[e] = r;
    if (two) x1[e] = r;
  }
}
}  // namespace ifx

extern "C" int ifx_magi_integrate(const ifx_magi_integrate_desc* d, void* stream) {
  IFX_REQUIRE(d && d->x, "ifx_magi_integrate: null descriptor or x");
  IFX_REQUIRE(d->n_chunks >= 0 && d->n_chunks <= IFX_MAGI_INTEGRATE_MAX_CHUNKS,
              "ifx_magi_integrate: %d chunks in the window, at most %d are built", d->n_chunks, IFX_MAGI_INTEGRATE_MAX_CHUNKS);
  IFX_REQUIRE(d->rows == 1 || d->rows == 2, "ifx_magi_integrate: rows %d (1 or 2)", d->rows);
  IFX_REQUIRE(d->channels > 0 && d->frame_elems > 0 && d->chunk_width > 0 && d->chunk_start >= 0 && d->frames > 0,
              "ifx_magi_integrate: bad geometry (channels %d, H W %d, chunk_width %d, chunk_start %d)", d->channels, d->frame_elems,
              d->chunk_width, d->chunk_start);
  IFX_REQUIRE(((int64_t)d->chunk_start + d->n_chunks) * d->chunk_width <= d->frames,
              "ifx_magi_integrate: window chunks [%d, %d) x %d frames run past the clip's %d frames", d->chunk_start,
              d->chunk_start + d->n_chunks, d->chunk_width, d->frames);
  IFX_REQUIRE(d->chan_stride >= (int64_t)d->frames * d->frame_elems && (d->rows == 1 || d->row_stride >= d->chan_stride * d->channels),
              "ifx_magi_integrate: x strides smaller than the block they step over");
  IFX_REQUIRE(!((uintptr_t)d->x & 3), "ifx_magi_integrate: x is not 4-byte aligned");
  IFX_REQUIRE(d->n_src >= 1 && d->n_src <= IFX_MAGI_INTEGRATE_MAX_SOURCES, "ifx_magi_integrate: %d sources (1 .. %d)", d->n_src,
              IFX_MAGI_INTEGRATE_MAX_SOURCES);
  IntegrateArgs a{};
  a.x = d->x, a.row_stride = d->row_stride, a.chan_stride = d->chan_stride;
  a.rows = d->rows, a.n_chunks = d->n_chunks, a.n_src = d->n_src;
  a.span = (long)d->chunk_width * d->frame_elems;
  a.x_first = (long)d->chunk_start * a.span;
  for (int c = 0; c < d->n_chunks; ++c) a.dt[c] = d->dt[c];
  for (int i = 0; i < d->n_src; ++i) {
    const ifx_magi_integrate_src& s = d->src[i];
    IFX_REQUIRE(s.v && !((uintptr_t)s.v & 3) && s.frames > 0 && s.chan_stride >= (int64_t)s.frames * d->frame_elems,
                "ifx_magi_integrate: source %d: null, misaligned or channel stride smaller than its frames", i);
    IFX_REQUIRE(s.first_chunk >= 0 && s.last_chunk >= s.first_chunk && s.last_chunk < (d->n_chunks > 0 ? d->n_chunks : 1),
                "ifx_magi_integrate: source %d covers window chunks %d .. %d of %d", i, s.first_chunk, s.last_chunk, d->n_chunks);
    IFX_REQUIRE(i > 0 || (s.first_chunk == 0 && s.last_chunk == (d->n_chunks > 0 ? d->n_chunks - 1 : 0)),
                "ifx_magi_integrate: source 0 must cover every chunk of the window");
    IFX_REQUIRE(s.first_frame >= 0 && (int64_t)s.first_frame + (int64_t)(s.last_chunk - s.first_chunk + 1) * d->chunk_width <= s.frames,
                "ifx_magi_integrate: source %d: frames [%d, +%d chunks) run past its %d frames", i, s.first_frame,
                s.last_chunk - s.first_chunk + 1, s.frames);
    a.v[i] = s.v, a.v_chan_stride[i] = s.chan_stride, a.v_first[i] = (long)s.first_frame * d->frame_elems;
    a.c0[i] = s.first_chunk, a.c1[i] = s.last_chunk;
    for (int c = 0; c < d->n_chunks; ++c) a.w[i][c] = s.w[c];
  }
  if (d->n_chunks == 0) return IFX_OK;
  const long spans = (long)d->channels * d->n_chunks;
  IFX_REQUIRE(spans <= 65535, "ifx_magi_integrate: channels x chunks = %ld spans exceed the grid's 65535", spans);
  // memory-bound: about eight workgroups per CU in all, the rest of a span by grid stride
  long gx = (a.span / 4 + 255) / 256, cap = 2048 / spans;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(magi_integrate_kernel, dim3((unsigned)gx, (unsigned)spans), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_magi_integrate");
}

extern "C" int ifx_act_rows(const ifx_bf16* x, ifx_bf16* y, int64_t n, int32_t mode, void* stream) {
  IFX_REQUIRE(x && y && n >= 0 && (mode == IFX_ACT_SILU || mode == IFX_ACT_TANH), "ifx_act_rows: bad arguments (mode %d)", mode);
  if (n == 0) return IFX_OK;
  hipLaunchKernelGGL(act_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, mode);
  return check_launch("ifx_act_rows");
}

extern "C" int ifx_silu_and_mul(const ifx_bf16* x, int32_t ldx, ifx_bf16* y, int32_t ldy, void* q, int32_t ldq, const float* divisor,
                                int32_t divisor_len, int32_t rows, int32_t f, void* stream) {
  IFX_REQUIRE(x && rows >= 0, "ifx_silu_and_mul: bad x / rows (%d)", rows);
  IFX_REQUIRE(f > 0 && f % 8 == 0, "ifx_silu_and_mul: f (%d) must be a positive multiple of 8", f);
  IFX_REQUIRE(y || q, "ifx_silu_and_mul: neither y nor q given: one output at least");
  IFX_REQUIRE(ldx >= 2 * (int64_t)f && ldx % 8 == 0, "ifx_silu_and_mul: ldx (%d) must be >= 2 * f (%d) and a multiple of 8", ldx, f);
  if (y) IFX_REQUIRE(ldy >= f && ldy % 8 == 0, "ifx_silu_and_mul: ldy (%d) must be >= f (%d) and a multiple of 8", ldy, f);
  if (q) IFX_REQUIRE(ldq >= f && ldq % 8 == 0, "ifx_silu_and_mul: ldq (%d) must be >= f (%d) and a multiple of 8", ldq, f);
  IFX_REQUIRE((q != nullptr) == (divisor != nullptr), "ifx_silu_and_mul: divisor goes with q (q %s, divisor %s)", q ? "given" : "NULL",
              divisor ? "given" : "NULL");
  if (q) IFX_REQUIRE(divisor_len == 1 || divisor_len == f, "ifx_silu_and_mul: divisor_len %d must be 1 or f (%d)", divisor_len, f);
  IFX_REQUIRE(!((uintptr_t)x & 15) && !((uintptr_t)y & 15) && !((uintptr_t)q & 7) && !((uintptr_t)divisor & 15),
              "ifx_silu_and_mul: x, y and divisor 16-byte aligned, q 8-byte aligned");
  if (rows == 0) return IFX_OK;
  const long chunks = (long)rows * (f / 8);
  const unsigned blocks = (unsigned)((chunks + 255) / 256 < 2048 ? (chunks + 255) / 256 : 2048);     // 8 blocks per CU, grid-stride beyond
  hipLaunchKernelGGL(silu_and_mul_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, (unsigned char*)q, ldq, divisor,
                     divisor_len == 1 ? 0 : 1, rows, f);
  return check_launch("ifx_silu_and_mul");
}

extern "C" int ifx_quant_static(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, const float* divisor, int32_t divisor_len,
                                float* row_scale, int32_t rows, int32_t K, int32_t format, int32_t via_bf16, void* stream) {
  IFX_REQUIRE(x && q && divisor && rows >= 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldq % 8 == 0,
              "ifx_quant_static: bad arguments (K %d)", K);
  IFX_REQUIRE(divisor_len == 1 || divisor_len == K, "ifx_quant_static: divisor_len %d must be 1 or K (%d)", divisor_len, K);
  IFX_REQUIRE(format == IFX_Q_FP8_E4M3 || format == IFX_Q_INT8, "ifx_quant_static: unknown format %d", format);
  IFX_REQUIRE(ldx >= K && ldq >= K, "ifx_quant_static: ldx (%d) and ldq (%d) must be >= K (%d)", ldx, ldq, K);
  if (rows == 0) return IFX_OK;
  return dispatch_q8_format(format, [&](auto fp8) {
    return launch_rows("ifx_quant_static", quant_static_kernel<decltype(fp8)::value>, rows, stream, x, ldx, (unsigned char*)q, ldq, divisor,
                       divisor_len == 1 ? 1 : 0, (const unsigned*)nullptr, row_scale, rows, K, via_bf16 ? 1 : 0);
  });
}

extern "C" int ifx_quant_per_tensor(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, float* row_scale, void* amax_workspace,
                                    int32_t rows, int32_t K, int32_t format, void* stream) {
  IFX_REQUIRE(x && q && row_scale && amax_workspace && rows >= 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldq % 8 == 0,
              "ifx_quant_per_tensor: bad arguments (K %d)", K);
  IFX_REQUIRE(format == IFX_Q_FP8_E4M3 || format == IFX_Q_INT8, "ifx_quant_per_tensor: unknown format %d", format);
  IFX_REQUIRE(ldx >= K && ldq >= K, "ifx_quant_per_tensor: ldx (%d) and ldq (%d) must be >= K (%d)", ldx, ldq, K);
  if (rows == 0) return IFX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(amax_workspace, 0, 4, s) != hipSuccess) {
    set_error("ifx_quant_per_tensor: hipMemsetAsync failed");
    return IFX_ELAUNCH;
  }
  const long chunks = (long)rows * (K / 8);
  const int blocks = (int)((chunks + 255) / 256 < 1024 ? (chunks + 255) / 256 : 1024);
  hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, rows, K, (unsigned*)amax_workspace);
  return dispatch_q8_format(format, [&](auto fp8) {
    return launch_rows("ifx_quant_per_tensor", quant_static_kernel<decltype(fp8)::value>, rows, stream, x, ldx, (unsigned char*)q, ldq,
                       (const float*)nullptr, 2, (const unsigned*)amax_workspace, row_scale, rows, K, 0);
  });
}

// The copies around VideoDiTModel's patch embedding and behind its final linear (inferix/models/magi/dit/dit_model.py:111-135 and
// :97-107), each one launch instead of a chain of torch copies (mul, cat, float, an 8-D permute, reshape).  Pure data movement with one
// rounding per element, HBM-bound (config 5: 12 MB of latents per forward).
//   magi_patch_rows_kernel : latents [N, C, T, H, W] -> fp32 rows [N T'H'W', C' pT pH pW], the A operand of the patch embedding's GEMM
//                            in the column order of weight.reshape(hidden, -1).  A lane reads along W, the contiguous axis of the
//                            latents: four elements (16 bytes of fp32, 8 of bf16) where every kept row starts on such a boundary and
//                            holds a multiple of four, one element otherwise (odd widths, a dropped trailing column).  The elements of
//                            one patch row are neighbours in the token row, so an even patch width stores them in 8-byte pairs.
//                            x_rescale_factor is applied in the input's dtype (a bf16 product is rounded to bf16 before it widens), the
//                            half_channel_vae copy is a second store of the same registers at column + C pT pH pW.
//   magi_unpatch_kernel    : fp32 [S, N, pT pH pW C] -> [N, C_out, T pT, H pH, W pW].  A lane writes along W of the result (16 bytes where
//                            the rows allow, else 4) and gathers its elements from the token rows; channels >= C_out are never read.
//                            The quotient is what torch's true divide by a host scalar computes on the device: the product with the
//                            fp32 reciprocal of the divisor, formed once on the host.
namespace ifx {
struct MagiPatchArgs {
  const void* x;
  float* rows;
  long long sn, sc, st, sh;          // element strides of the latents (W stride 1)
  long long units;                   // per (n, c): Tk Hk Wk / 4 (vector path) or Tk Hk Wk
  long long ld, tokens, dup_cols;    // dup_cols: C pT pH pW with the half_channel_vae copy, else 0
  int C, Hk, Wk, pT, pH, pW, lH, lW; // Hk, Wk: kept extents (whole patches); lH, lW: patches per column / row
  int pair;                          // vector path: 8-byte stores (pW even, ld even)
  float scale;
};

template <bool BF, bool VEC>
__global__ __launch_bounds__(256) void magi_patch_rows_kernel(MagiPatchArgs A) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= A.units) return;
  const int n = blockIdx.y / A.C, c = blockIdx.y - n * A.C;
  const int per_row = VEC ? A.Wk >> 2 : A.Wk;
  const long long r = u / per_row;
  const int w = (int)(u - r * per_row) * (VEC ? 4 : 1);
  const int t = (int)(r / A.Hk), h = (int)(r - (long long)t * A.Hk);
  const long long src = n * A.sn + c * A.sc + t * A.st + h * A.sh + w;
  constexpr int NV = VEC ? 4 : 1;
  float v[NV];
  if constexpr (BF) {
    const unsigned short* p = static_cast<const unsigned short*>(A.x) + src;
    unsigned short raw[NV];
    if constexpr (VEC) {
      const u16x4 q = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) raw[j] = q[j];
    } else {
      raw[0] = *p;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = rbf(bf2f(raw[j]) * A.scale);           // the bf16 tensor product, then .float()
  } else {
    const float* p = static_cast<const float*>(A.x) + src;
    if constexpr (VEC) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = q[j] * A.scale;
    } else {
      v[0] = *p * A.scale;
    }
  }
  const int lt = t / A.pT, at = t - lt * A.pT, lh = h / A.pH, ah = h - lh * A.pH;
  const long long row0 = (long long)n * A.tokens + ((long long)lt * A.lH + lh) * A.lW;
  const long long col0 = (((long long)c * A.pT + at) * A.pH + ah) * A.pW;
  if (VEC && A.pair) {
#pragma unroll
    for (int j = 0; j < NV; j += 2) {
      const int lw = (w + j) / A.pW, aw = (w + j) - lw * A.pW;
      float* d = A.rows + (row0 + lw) * A.ld + col0 + aw;
      const float2 o = make_float2(v[j], v[j + (VEC ? 1 : 0)]);
      *reinterpret_cast<float2*>(d) = o;
      if (A.dup_cols) *reinterpret_cast<float2*>(d + A.dup_cols) = o;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int lw = (w + j) / A.pW, aw = (w + j) - lw * A.pW;
    float* d = A.rows + (row0 + lw) * A.ld + col0 + aw;
    *d = v[j];
    if (A.dup_cols) d[A.dup_cols] = v[j];
  }
}

struct MagiUnpatchArgs {
  const float* o;
  float* out;
  long long tok_stride, K;           // elements between tokens (N K) and between the samples of one token (K)
  long long units;                   // per (n, c): To Ho Wo / 4 (vector path) or To Ho Wo
  long long plane_rows;              // To Ho
  int C, c_out, Ho, Wo, pT, pH, pW, lH, lW;
  float inv;
};

template <bool VEC>
__global__ __launch_bounds__(256) void magi_unpatch_kernel(MagiUnpatchArgs A) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= A.units) return;
  const int n = blockIdx.y / A.c_out, c = blockIdx.y - n * A.c_out;
  const int per_row = VEC ? A.Wo >> 2 : A.Wo;
  const long long r = u / per_row;
  const int w = (int)(u - r * per_row) * (VEC ? 4 : 1);
  const int t = (int)(r / A.Ho), h = (int)(r - (long long)t * A.Ho);
  const int lt = t / A.pT, at = t - lt * A.pT, lh = h / A.pH, ah = h - lh * A.pH;
  const long long tok0 = ((long long)lt * A.lH + lh) * A.lW;
  const float* src = A.o + n * A.K + ((long long)(at * A.pH + ah) * A.pW) * A.C + c;
  constexpr int NV = VEC ? 4 : 1;
  float v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int lw = (w + j) / A.pW, aw = (w + j) - lw * A.pW;
    v[j] = src[(tok0 + lw) * A.tok_stride + (long long)aw * A.C] * A.inv;
  }
  float* d = A.out + ((long long)blockIdx.y * A.plane_rows + r) * A.Wo + w;      // plane (n, c) of the contiguous result
  if constexpr (VEC) {
    f32x4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = v[j];
    *reinterpret_cast<f32x4*>(d) = q;
  } else {
    *d = v[0];
  }
}
}  // namespace ifx

extern "C" int ifx_magi_patch_rows(const void* x, int32_t is_bf16, const int64_t* dims, const int64_t* strides, float scale,
                                   int32_t duplicate, int32_t patch_t, int32_t patch_h, int32_t patch_w, float* rows, int64_t ld,
                                   void* stream) {
  IFX_REQUIRE(x && dims && strides && rows, "ifx_magi_patch_rows: null argument");
  IFX_REQUIRE(patch_t >= 1 && patch_h >= 1 && patch_w >= 1 && patch_t <= 64 && patch_h <= 64 && patch_w <= 64,
              "ifx_magi_patch_rows: bad patch %d x %d x %d", patch_t, patch_h, patch_w);
  const long long N = dims[0], Cc = dims[1], T = dims[2], H = dims[3], W = dims[4];
  IFX_REQUIRE(N >= 1 && Cc >= 1 && T >= 0 && H >= 0 && W >= 0 && T <= 0x7fffffffLL && H <= 0x7fffffffLL && W <= 0x7fffffffLL &&
                  N * Cc <= 65535,
              "ifx_magi_patch_rows: latent dims [%lld, %lld, %lld, %lld, %lld] (N C in 1 .. 65535)", N, Cc, T, H, W);
  IFX_REQUIRE(strides[4] == 1, "ifx_magi_patch_rows: the W stride must be 1, got %lld", (long long)strides[4]);
  for (int a = 0; a < 4; ++a)
    IFX_REQUIRE(strides[a] >= 0, "ifx_magi_patch_rows: stride %d is negative (%lld)", a, (long long)strides[a]);
  const long long lT = T / patch_t, lH = H / patch_h, lW = W / patch_w;
  const long long Kc = Cc * patch_t * patch_h * patch_w, K = duplicate ? 2 * Kc : Kc;
  IFX_REQUIRE(ld >= K, "ifx_magi_patch_rows: a patch row of %lld elements does not fit ld (%lld)", K, (long long)ld);
  const int esz = is_bf16 ? 2 : 4;
  IFX_REQUIRE((uintptr_t)rows % 4 == 0 && (uintptr_t)x % esz == 0, "ifx_magi_patch_rows: rows must be 4-byte aligned, x %d-byte", esz);
  const long long tokens = lT * lH * lW;
  IFX_REQUIRE(N * tokens <= 0x7fffffffLL, "ifx_magi_patch_rows: %lld token rows", N * tokens);
  if (tokens == 0) return IFX_OK;
  const long long Tk = lT * patch_t, Hk = lH * patch_h, Wk = lW * patch_w;
  // four elements per lane where every kept row starts on a 4-element boundary of an aligned base and holds whole groups of four
  const bool vec = Wk % 4 == 0 && strides[0] % 4 == 0 && strides[1] % 4 == 0 && strides[2] % 4 == 0 && strides[3] % 4 == 0 &&
                   (uintptr_t)x % (4 * esz) == 0;
  ifx::MagiPatchArgs a{};
  a.x = x, a.rows = rows;
  a.sn = strides[0], a.sc = strides[1], a.st = strides[2], a.sh = strides[3];
  a.units = Tk * Hk * (vec ? Wk / 4 : Wk);
  a.ld = ld, a.tokens = tokens, a.dup_cols = duplicate ? Kc : 0;
  a.C = (int)Cc, a.Hk = (int)Hk, a.Wk = (int)Wk, a.pT = patch_t, a.pH = patch_h, a.pW = patch_w, a.lH = (int)lH, a.lW = (int)lW;
  a.pair = vec && patch_w % 2 == 0 && ld % 2 == 0 && (uintptr_t)rows % 8 == 0;
  a.scale = scale;
  const long long blocks = (a.units + 255) / 256;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_magi_patch_rows: launch too large");
  const dim3 grid((unsigned)blocks, (unsigned)(N * Cc));
  hipStream_t s = (hipStream_t)stream;
  if (is_bf16) {
    if (vec) hipLaunchKernelGGL((ifx::magi_patch_rows_kernel<true, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ifx::magi_patch_rows_kernel<true, false>), grid, dim3(256), 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((ifx::magi_patch_rows_kernel<false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ifx::magi_patch_rows_kernel<false, false>), grid, dim3(256), 0, s, a);
  }
  return check_launch("ifx_magi_patch_rows");
}

extern "C" int ifx_magi_unpatch(const float* o, int64_t ld_token, int32_t batch, int32_t channels, int32_t c_out, int32_t lat_t,
                                int32_t lat_h, int32_t lat_w, int32_t patch_t, int32_t patch_h, int32_t patch_w, float divisor, float* out,
                                void* stream) {
  IFX_REQUIRE(o && out, "ifx_magi_unpatch: null argument");
  IFX_REQUIRE(patch_t >= 1 && patch_h >= 1 && patch_w >= 1 && patch_t <= 64 && patch_h <= 64 && patch_w <= 64,
              "ifx_magi_unpatch: bad patch %d x %d x %d", patch_t, patch_h, patch_w);
  IFX_REQUIRE(batch >= 1 && channels >= 1 && c_out >= 1 && c_out <= channels && (long long)batch * c_out <= 65535,
              "ifx_magi_unpatch: batch %d, channels %d, c_out %d (1 <= c_out <= channels, batch x c_out <= 65535)", batch, channels, c_out);
  IFX_REQUIRE(lat_t >= 0 && lat_h >= 0 && lat_w >= 0, "ifx_magi_unpatch: latent shape %d x %d x %d", lat_t, lat_h, lat_w);
  const long long K = (long long)patch_t * patch_h * patch_w * channels;
  IFX_REQUIRE(ld_token >= (long long)batch * K, "ifx_magi_unpatch: ld_token (%lld) is smaller than batch x K = %d x %lld",
              (long long)ld_token, batch, K);
  IFX_REQUIRE(divisor != 0.f, "ifx_magi_unpatch: divisor 0");
  IFX_REQUIRE((uintptr_t)o % 4 == 0 && (uintptr_t)out % 4 == 0, "ifx_magi_unpatch: o / out must be 4-byte aligned");
  const long long To = (long long)lat_t * patch_t, Ho = (long long)lat_h * patch_h, Wo = (long long)lat_w * patch_w;
  IFX_REQUIRE(Ho <= 0x7fffffffLL && Wo <= 0x7fffffffLL && To * Ho <= 0x7fffffffLL, "ifx_magi_unpatch: result %lld x %lld x %lld", To, Ho, Wo);
  if (To * Ho * Wo == 0) return IFX_OK;
  const bool vec = Wo % 4 == 0 && (uintptr_t)out % 16 == 0;
  ifx::MagiUnpatchArgs a{};
  a.o = o, a.out = out, a.tok_stride = ld_token, a.K = K;
  a.plane_rows = To * Ho;
  a.units = a.plane_rows * (vec ? Wo / 4 : Wo);
  a.C = channels, a.c_out = c_out, a.Ho = (int)Ho, a.Wo = (int)Wo, a.pT = patch_t, a.pH = patch_h, a.pW = patch_w, a.lH = lat_h, a.lW = lat_w;
  a.inv = 1.0f / divisor;
  const long long blocks = (a.units + 255) / 256;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_magi_unpatch: launch too large");
  const dim3 grid((unsigned)blocks, (unsigned)(batch * c_out));
  if (vec) hipLaunchKernelGGL(ifx::magi_unpatch_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(ifx::magi_unpatch_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_magi_unpatch");
}

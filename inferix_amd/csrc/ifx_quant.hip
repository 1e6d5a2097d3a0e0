// Dynamic 8-bit linear layers (gfx950): per-token activation quantisation + FP8 (OCP e4m3) / INT8 MFMA GEMM
// with per-token x per-channel dequantisation and the block's fused epilogues.
//
// Replaces the DAX `quantize_dynamic` linears the reference wires in
// example/quantization/run_self_forcing_quantized.py:19-23,47-64 (dynamic per-token activation x per-channel
// weight, FP8 or INT8).  DAX is an un-vendored, unpinned dependency: its arithmetic is NOT in the reference tree,
// so the scheme is defined here (and restated in oracle/quant_oracle.py) — parity with DAX itself is unpinned:
//
//   s_a[m] = max_k |x[m,k]| / QMAX          (fp32; 1.0 for an all-zero row)      QMAX = 448 (e4m3) | 127 (int8)
//   xq[m,k] = cast( clamp(x[m,k] / s_a[m], +-QMAX) )      e4m3: round-to-nearest-even ; int8: rint
//   s_w[n], wq[n,k] : the same per OUTPUT channel of W, computed once when the module is quantised
//   y[m,n]  = epilogue( bf16( acc[m,n] * (s_a[m] * s_w[n]) + bias[n] ) )         acc: fp32 (fp8) / exact int32 (int8)
//
// Kernels:
//   quant_rows_kernel : one wavefront per token row, two passes over the row (abs-max, then scale+cast; the second
//                       pass hits L2), 16-byte loads, 8-byte stores: HBM-bound (reads 2 B, writes 1 B per element).
//                       Rows up to 9216 wide stay in registers and go through quant_row_dynamic of ifx_rows.h, the quantiser
//                       that LayerNorm fuses too: its rounding is changed there, once.
//   gemm_q8_kernel    : 128 x 128 x 128(bytes of K) tiles, 4 waves, 2x2 fragments of 32x32 per wave;
//                       v_mfma_f32_32x32x16_fp8_fp8 (two per 16-byte fragment read) or v_mfma_i32_32x32x32_i8;
//                       operands staged global -> registers -> LDS (double buffered), 128-byte rows with the
//                       16-byte chunk index XOR ((row >> 1) & 7): conflict-free ds_read_b128 for 32-row fragments;
//                       half the operand bytes of the bf16 kernel per FLOP.
#include "ifx_gemm_tile.h"
#include "ifx_rows.h"

namespace ifx {

typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) long i64x2;

// ---------------------------------------------------------------------------------------------------------
// NCH = ceil(K / 512) chunks of 8 elements per lane: the whole row is loaded ONCE with all its 16-byte loads in flight
// (NCH <= 18, K <= 9216 — the 8960-wide FFN activations); NCH == 0 is the generic two-pass loop for wider rows.
template <bool FP8, int NCH>
__global__ __launch_bounds__(256) void quant_rows_kernel(const unsigned short* __restrict__ x, int ldx,
                                                         unsigned char* __restrict__ q, int ldq,
                                                         float* __restrict__ scale, int rows, int K) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const unsigned short* xr = x + (size_t)r * ldx;
  unsigned char* qr = q + (size_t)r * ldq;
  if constexpr (NCH > 0) {
    u16x8 u[NCH > 0 ? NCH : 1];
    load_chunks<NCH>(u, xr, K, lane);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c * 512 + lane * 8 >= K) u[c] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    quant_row_dynamic<FP8, NCH>(u, qr, scale + r, K, lane);
    return;
  }
  constexpr float QMAX = FP8 ? 448.0f : 127.0f;
  float amax = 0.f;
  for (int col = lane * 8; col < K; col += 512) {
    const u16x8 u = *reinterpret_cast<const u16x8*>(xr + col);
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(u[i])));
  }
  amax = wave_max(amax);
  const float s = amax > 0.f ? amax / QMAX : 1.0f;
  if (lane == 0) scale[r] = s;
  for (int col = lane * 8; col < K; col += 512) {
    const u16x8 u = *reinterpret_cast<const u16x8*>(xr + col);
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = fminf(fmaxf(bf2f(u[i]) / s, -QMAX), QMAX);
    *reinterpret_cast<u32x2*>(qr + col) = pack8<FP8>(v);
  }
}

// ---------------------------------------------------------------------------------------------------------
// div_clamp_to (dit_module.py:367-387) of four bf16 values -> four e4m3 bytes
__device__ __forceinline__ unsigned quant4_e4m3(const float (&x)[4], const f32x4 d, int via_bf16) {
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = fminf(fmaxf(x[e] / d[e], -448.0f), 448.0f);
    v[e] = via_bf16 ? rbf(t) : t;
  }
  unsigned w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], w, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w, true);
}

template <bool FP8, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_q8_kernel(const unsigned char* __restrict__ x, int ldx,
                                                         const unsigned char* __restrict__ w,
                                                         unsigned short* __restrict__ y, int ldy, int M, int N, int K,
                                                         int tiles_m, int tiles_n, EpiArgsQ ea) {
  constexpr int BM = 128, BN = 128, BKB = 128;   // K tile = 128 one-byte elements
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int total = tiles_m * tiles_n, per_xcd = (total + 7) / 8;
  const int t_id = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per_xcd || t_id >= total) return;
  const TileOrigin org = tile_origin_of<BM, BN, 8>(t_id, tiles_m, tiles_n);
  const int m_base = org.m, n_base = org.n;

  const unsigned char* gx[4];
  const unsigned char* gw[4];
  int lds_off[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int qi = tid + 256 * p, row = qi >> 3, c = qi & 7;
    gx[p] = x + (size_t)min(m_base + row, M - 1) * ldx + c * 16;
    gw[p] = w + (size_t)min(n_base + row, N - 1) * K + c * 16;
    lds_off[p] = row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
  }
  u32x4 rx[4], rw[4];
  auto gload = [&](int kt) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      rx[p] = *reinterpret_cast<const u32x4*>(gx[p] + (size_t)kt * BKB);
      rw[p] = *reinterpret_cast<const u32x4*>(gw[p] + (size_t)kt * BKB);
    }
  };
  auto lstore = [&](int buf) {
    unsigned char* bx = smem + buf * 32768;
    unsigned char* bw = bx + 16384;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *reinterpret_cast<u32x4*>(bx + lds_off[p]) = rx[p];
      *reinterpret_cast<u32x4*>(bw + lds_off[p]) = rw[p];
    }
  };

  f32x16 facc[2][2];
  i32x16 iacc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        facc[i][j][r] = 0.f;
        iacc[i][j][r] = 0;
      }

  const int KT = K / BKB;
  gload(0);
  lstore(0);
  __syncthreads();
  const int l31 = lane & 31, hi = lane >> 5;
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) gload(kt + 1);
    const unsigned char* bx = smem + buf * 32768;
    const unsigned char* bw = bx + 16384;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = 2 * p + hi;
      i32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wn * 64 + i * 32 + l31;
        a[i] = *reinterpret_cast<const i32x4*>(bw + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = wm * 64 + j * 32 + l31;
        b[j] = *reinterpret_cast<const i32x4*>(bx + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (FP8) {
            // one 16-byte fragment = two K=16 steps; the k-slot relabelling is the same for both operands
            const i64x2 al = __builtin_bit_cast(i64x2, a[i]), bl = __builtin_bit_cast(i64x2, b[j]);
            facc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[0], bl[0], facc[i][j], 0, 0, 0);
            facc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[1], bl[1], facc[i][j], 0, 0, 0);
          } else {
            iacc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], iacc[i][j], 0, 0, 0);
          }
        }
    }
    if (kt + 1 < KT) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds D[n = n0 + 32i + 8g + 4hi + e][m = m0 + 32j + l31]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m_base + wm * 64 + j * 32 + l31;
    if (m >= M) continue;
    const float sa = ea.sa[m];
    const unsigned short* gate_row = nullptr;
    if (EPI == IFX_EPI_GATE_RES)
      gate_row = ea.mod + ((size_t)(m / ea.rows_per_group) * ea.mod_slots + ea.gate_slot) * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n_base + wn * 64 + i * 32 + g * 8 + hi * 4;
        if (n >= N) continue;
        const f32x4 swv = *reinterpret_cast<const f32x4*>(ea.sw + n);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float acc = FP8 ? facc[i][j][4 * g + e] : (float)iacc[i][j][4 * g + e];
          v[e] = acc * (sa * swv[e]);
        }
        if (ea.bias) {
          const u16x4 bv = *reinterpret_cast<const u16x4*>(ea.bias + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bf2f(bv[e]);
        }
        u16x4 vb, rv = {}, gv = {};
#pragma unroll
        for (int e = 0; e < 4; ++e) vb[e] = f2bf(v[e]);
        if (EPI == IFX_EPI_RESIDUAL || EPI == IFX_EPI_GATE_RES)
          rv = *reinterpret_cast<const u16x4*>(ea.residual + (size_t)m * ea.ld_res + n);
        if (EPI == IFX_EPI_GATE_RES) gv = *reinterpret_cast<const u16x4*>(gate_row + n);
        const u16x4 o = epi_combine<EPI, 4>(vb, rv, gv, ea.gelu_erf());
        if (EPI == IFX_EPI_GELU_TANH && ea.qdiv != nullptr) {
          const float ob[4] = {bf2f(o[0]), bf2f(o[1]), bf2f(o[2]), bf2f(o[3])};
          *reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(y) + (size_t)m * ldy + n) =
              quant4_e4m3(ob, *reinterpret_cast<const f32x4*>(ea.qdiv + n), ea.q_via_bf16);
        } else {
          *reinterpret_cast<u16x4*>(y + (size_t)m * ldy + n) = o;
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------------------
// LDS-DMA variant for the large shapes: BM x BN tiles, K-steps of 64 one-byte elements, 8 waves, 4-stage ring of
// 64-byte rows — byte for byte the geometry of the bf16 K=32 kernel (ifx_gemm_glds.hip: gemm_big_kernel), so the DMA
// map, the chunk swizzle ((row >> 2) & 3), the fragment reads and the LDS-transposed epilogue are the same; per FLOP it
// moves half the operand bytes, which is what bounds the bf16 GEMMs (profiles/r1d_gemm_ablation.md).
//   FP8 : PP_F8F6F4 = 1 -> one v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales) per 32-byte fragment pair: the 5 PFLOP/s
//         instruction; 0 -> four v_mfma_f32_32x32x16_fp8_fp8.     INT8: two v_mfma_i32_32x32x32_i8.
// The K order inside a fragment is whatever the hardware uses — both operands are read with the same lane -> byte map,
// and a dot product does not care about a common permutation of k.
#ifndef IFX_Q8_F8F6F4
#define IFX_Q8_F8F6F4 1
#endif
typedef __attribute__((ext_vector_type(8))) int i32x8;

// BKB = bytes of K per operand row of a stage: 64 (four stages) or 128 (two / three stages).  LDS-DMA moves rows of >= 128 B from L2 at
// twice the rate of 64-byte rows (tools/probe_dma.hip), the same finding that moved the bf16 256x256 tile to 64-deep stages.
template <bool FP8, int BM, int BN, int WAVES_M, int EPI, int BKB = 64, int NST = 4>
__global__ __launch_bounds__(512) void gemm_q8_dma_kernel(const unsigned char* __restrict__ x, int ldx,
                                                          const unsigned char* __restrict__ w,
                                                          unsigned short* __restrict__ y, int ldy, int M, int N, int K,
                                                          int tiles_m, int total, int per_xcd, EpiArgsQ ea) {
  constexpr int CPR = BKB / 16, RPP = 64 / CPR;           // 16-byte chunks per row (4 | 8), rows per 1 KiB DMA piece (16 | 8)
  constexpr int SW_SH = BKB == 64 ? 2 : 1;                 // swizzle phase: (row >> SW_SH) & (CPR - 1)
  constexpr int STAGE = (BM + BN) * BKB;
  constexpr int A_OFF = 0, B_OFF = BM * BKB;
  constexpr int WAVES_N = 8 / WAVES_M;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, TJ = WM / 32, TI = WN / 32;
  constexpr int PA = BM / (8 * RPP), PB = BN / (8 * RPP), P = PA + PB;
  static_assert((NST - 2) * P <= 63 && NST >= 2 && NST <= 4, "stages");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xcd = blockIdx.x & 7, slot_i = blockIdx.x >> 3;
  const int t_id = xcd * per_xcd + slot_i;
  if (slot_i >= per_xcd || t_id >= total) return;
  const TileOrigin org = tile_origin<BM, BN, 4>(t_id, tiles_m, total);
  const int m_base = org.m, n_base = org.n;
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;

  const int r16 = lane / CPR, pc = lane % CPR;
  const unsigned char* src_a[PA];
  const unsigned char* src_b[PB];
#pragma unroll
  for (int r = 0; r < PA; ++r) {
    const int row = (r * 8 + wave) * RPP + r16;
    src_a[r] = x + (size_t)min(m_base + row, M - 1) * ldx + (pc ^ ((row >> SW_SH) & (CPR - 1))) * 16;
  }
#pragma unroll
  for (int r = 0; r < PB; ++r) {
    const int row = (r * 8 + wave) * RPP + r16;
    src_b[r] = w + (size_t)min(n_base + row, N - 1) * K + (pc ^ ((row >> SW_SH) & (CPR - 1))) * 16;
  }
  auto issue = [&](int kt) {
    unsigned char* st = smem + (kt % NST) * STAGE;
    const size_t ko = (size_t)kt * BKB;
#pragma unroll
    for (int r = 0; r < PA; ++r)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src_a[r] + ko), (lds_ptr_t)(st + A_OFF + (r * 8 + wave) * 1024), 16, 0, 0);
#pragma unroll
    for (int r = 0; r < PB; ++r)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(src_b[r] + ko), (lds_ptr_t)(st + B_OFF + (r * 8 + wave) * 1024), 16, 0, 0);
  };

  f32x16 facc[TI][TJ];
  i32x16 iacc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        facc[i][j][r] = 0.f;
        iacc[i][j][r] = 0;
      }

  const int KT = K / BKB;
#pragma unroll
  for (int i = 0; i < NST - 1; ++i)
    if (i < KT) issue(i);

  const int l31 = lane & 31, hi = lane >> 5;
  int a_off[TJ], b_off[TI], a_swz[TJ], b_swz[TI];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int row = wm * WM + j * 32 + l31;
    a_off[j] = A_OFF + row * BKB;
    a_swz[j] = (row >> SW_SH) & (CPR - 1);
  }
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int row = wn * WN + i * 32 + l31;
    b_off[i] = B_OFF + row * BKB;
    b_swz[i] = (row >> SW_SH) & (CPR - 1);
  }

  for (int kt = 0; kt < KT; ++kt) {
    const int later = min(KT - 1 - kt, NST - 2);
    if (later == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P) : "memory");
    else if (later == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + NST - 1 < KT) issue(kt + NST - 1);
    const unsigned char* st = smem + (kt % NST) * STAGE;
#pragma unroll
    for (int kh = 0; kh < BKB / 64; ++kh) {                // 64 bytes of K per MFMA step
    i32x4 fa[2][TJ], fb[2][TI];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = 4 * kh + 2 * ks + hi;
#pragma unroll
      for (int i = 0; i < TI; ++i) fb[ks][i] = *reinterpret_cast<const i32x4*>(st + b_off[i] + ((c ^ b_swz[i]) << 4));
#pragma unroll
      for (int j = 0; j < TJ; ++j) fa[ks][j] = *reinterpret_cast<const i32x4*>(st + a_off[j] + ((c ^ a_swz[j]) << 4));
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        if (FP8) {
#if IFX_Q8_F8F6F4
          const i32x8 av = __builtin_shufflevector(fb[0][i], fb[1][i], 0, 1, 2, 3, 4, 5, 6, 7);
          const i32x8 bv = __builtin_shufflevector(fa[0][j], fa[1][j], 0, 1, 2, 3, 4, 5, 6, 7);
          facc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, facc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
#else
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const i64x2 al = __builtin_bit_cast(i64x2, fb[ks][i]), bl = __builtin_bit_cast(i64x2, fa[ks][j]);
            facc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[0], bl[0], facc[i][j], 0, 0, 0);
            facc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(al[1], bl[1], facc[i][j], 0, 0, 0);
          }
#endif
        } else {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            iacc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fb[ks][i], fa[ks][j], iacc[i][j], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: v = bf16(acc * sa[m] * sw[n] + bias[n]) transposed through LDS per wave, then 16-byte row accesses
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  constexpr int RB = WN * 2, CR = RB / 16, RP = 64 / CR;
  unsigned char* tw = smem + wave * (WM * RB);
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int mrow = j * 32 + l31;
    const int m = m_base + wm * WM + mrow;
    const float sa = ea.sa[min(m, M - 1)];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int nl = i * 32 + g * 8 + hi * 4;
        const int n = n_base + wn * WN + nl;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (n < N) {
          const f32x4 swv = *reinterpret_cast<const f32x4*>(ea.sw + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float acc = FP8 ? facc[i][j][4 * g + e] : (float)iacc[i][j][4 * g + e];
            v[e] = acc * (sa * swv[e]);
          }
          if (ea.bias) {
            const u16x4 bv = *reinterpret_cast<const u16x4*>(ea.bias + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bf2f(bv[e]);
          }
        }
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
        const int chunk = (nl >> 3) ^ (mrow & (CR - 1));
        *reinterpret_cast<u16x4*>(tw + mrow * RB + chunk * 16 + (nl & 4) * 2) = o;
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  {
    const int rr = lane / CR, cc = lane % CR;
#pragma unroll
    for (int p = 0; p < WM / RP; ++p) {
      const int mrow = p * RP + rr;
      const int m = m_base + wm * WM + mrow;
      const int n = n_base + wn * WN + cc * 8;
      const u16x8 vv = *reinterpret_cast<const u16x8*>(tw + mrow * RB + ((cc ^ (mrow & (CR - 1))) << 4));
      if (m >= M || n >= N) continue;
      const u16x8 o = epi_apply<EPI, 8>(vv, m, n, N, ea);
      if (EPI == IFX_EPI_GELU_TANH && ea.qdiv != nullptr) {
        const float lo[4] = {bf2f(o[0]), bf2f(o[1]), bf2f(o[2]), bf2f(o[3])};
        const float hi4[4] = {bf2f(o[4]), bf2f(o[5]), bf2f(o[6]), bf2f(o[7])};
        const unsigned w0 = quant4_e4m3(lo, *reinterpret_cast<const f32x4*>(ea.qdiv + n), ea.q_via_bf16);
        const unsigned w1 = quant4_e4m3(hi4, *reinterpret_cast<const f32x4*>(ea.qdiv + n + 4), ea.q_via_bf16);
        *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned char*>(y) + (size_t)m * ldy + n) = u32x2{w0, w1};
      } else {
        *reinterpret_cast<u16x8*>(y + (size_t)m * ldy + n) = o;
      }
    }
  }
}

// the tile kind as launch_tile (ifx_gemm_tile.h) takes it
template <bool FP8, int BM_, int BN_, int WAVES_M, int BKB = 64, int NST = 4>
struct Q8DmaTile {
  static constexpr int BM = BM_, BN = BN_, THREADS = 512;
  static constexpr size_t RING = (size_t)NST * (BM + BN) * BKB;
  static_assert(RING <= 160 * 1024, "LDS");
  static constexpr size_t LDS = std::max(RING, (size_t)BM * BN * 2);     // operand ring / per-wave epilogue transposes
  static constexpr const char* NAME = "ifx_gemm_q8(dma)";
  template <int EPI>
  static constexpr auto kernel = gemm_q8_dma_kernel<FP8, BM, BN, WAVES_M, EPI, BKB, NST>;
};

}  // namespace ifx

using namespace ifx;

extern "C" int ifx_quant_per_token(const ifx_bf16* x, int32_t ldx, void* q, int32_t ldq, float* scale, int32_t rows,
                                   int32_t K, int32_t format, void* stream) {
  IFX_REQUIRE(x && q && scale && rows >= 0 && K > 0 && K % 8 == 0 && ldx % 8 == 0 && ldq % 8 == 0,
              "ifx_quant_per_token: bad arguments (K %d)", K);
  IFX_REQUIRE(ldx >= K && ldq >= K, "ifx_quant_per_token: row strides ldx (%d) and ldq (%d) must be >= K (%d)", ldx, ldq, K);
  IFX_REQUIRE(format == IFX_Q_FP8_E4M3 || format == IFX_Q_INT8, "ifx_quant_per_token: unknown format %d", format);
  if (rows == 0) return IFX_OK;
  return dispatch_nch<1, 3, 6, 10, 18, 0>(K, nullptr, [&](auto nch) {       // 0: the generic loop takes the rows wider than 9216
    return dispatch_q8_format(format, [&](auto fp8) {
      return launch_rows("ifx_quant_per_token", quant_rows_kernel<decltype(fp8)::value, decltype(nch)::value>, rows, stream, x, ldx,
                         (unsigned char*)q, ldq, scale, rows, K);
    });
  });
}

// Arguments checked, the call described (GemmRequest), gemm_q8_plan of ifx_gemm_plan.h decides, this launches.
static int gemm_q8_impl(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                        const ifx_bf16* bias, ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K,
                        int32_t format, const ifx_epilogue* epi, void* stream, const float* qdiv, int q_via_bf16,
                        void* workspace = nullptr, int64_t workspace_bytes = 0) {
  IFX_REQUIRE(xq && wq && x_scale && w_scale && y && M >= 0 && N > 0 && K > 0, "ifx_gemm_q8: null/empty operand");
  IFX_REQUIRE(K % 128 == 0, "ifx_gemm_q8: K (%d) must be a multiple of 128", K);
  IFX_REQUIRE(N % 4 == 0 && ldx % 16 == 0 && ldy % 4 == 0, "ifx_gemm_q8: N %% 4, ldx %% 16, ldy %% 4 required");
  IFX_REQUIRE(format == IFX_Q_FP8_E4M3 || format == IFX_Q_INT8, "ifx_gemm_q8: unknown format %d", format);
  if (qdiv != nullptr) {
    const int asked = epi ? epi->epilogue : IFX_EPI_BIAS;
    IFX_REQUIRE(asked == IFX_EPI_GELU_TANH || asked == IFX_EPI_GELU_ERF, "ifx_gemm_q8_quant_out: epilogue %d (a GELU epilogue feeds the "
                "quantised output)", asked);
    IFX_REQUIRE(ldy % 8 == 0, "ifx_gemm_q8_quant_out: ldyq (%d) must be a multiple of 8 bytes", ldy);
  }
  int mode;
  EpiArgsP ea;
  if (const int rc = resolve_epilogue(epi, bias, "ifx_gemm_q8", &mode, &ea)) return rc;
  ea.sa = x_scale, ea.sw = w_scale, ea.qdiv = qdiv, ea.q_via_bf16 = q_via_bf16;
  IFX_REQUIRE(epi == nullptr || epi->y2 == nullptr, "ifx_gemm_q8: the second destination (ifx_epilogue.y2) is built for the bf16 launches only");
  // base alignment: 16-byte chunks of xq / wq and four w_scale values per load in every kernel; bias, residual, gate rows and y in 8-byte
  // vectors in the register-staged kernel, 16-byte vectors (bias: 8) in the others
  IFX_REQUIRE(!(((uintptr_t)xq | (uintptr_t)wq | (uintptr_t)w_scale) & 15), "ifx_gemm_q8: xq, wq and w_scale must be 16-byte aligned");
  IFX_REQUIRE(!((uintptr_t)x_scale & 3) && !(((uintptr_t)y | (uintptr_t)bias | (uintptr_t)ea.residual | (uintptr_t)ea.mod) & 7),
              "ifx_gemm_q8: y, bias, residual and mod must be 8-byte aligned, x_scale 4-byte aligned");
  if (M == 0) return IFX_OK;
  hipStream_t s = (hipStream_t)stream;
  const unsigned char* xp = (const unsigned char*)xq;
  const unsigned char* wp = (const unsigned char*)wq;
  GemmRequest r = gemm_request(M, N, K, mode, ea, y, ldy, workspace, workspace_bytes);
  r.qdiv = qdiv != nullptr, r.qdiv16 = ((uintptr_t)qdiv & 15) == 0;
  const GemmPlan plan = gemm_q8_plan(r, gemm_variant(), gemm_small_split());
  if (plan.path == kGemmPathPp)
    return launch_gemm_pp((const unsigned short*)xp, ldx, (const unsigned short*)wp, y, ldy, M, N, K, mode, ea, s, plan.tj, plan.ks,
                          plan.ws_bytes > 0 ? workspace : nullptr, format == IFX_Q_INT8 ? 1 : 0);
  if (plan.path == kGemmPathLdsDma)
    return dispatch_q8_format(format, [&](auto fp8_c) {
      constexpr bool F = decltype(fp8_c)::value;
      const EpiArgsQ& eq = ea;
      auto run = [&](auto t) { return launch_tile<decltype(t)>(xp, ldx, wp, y, ldy, M, N, K, mode, eq, s); };
      switch (plan.tile) {
        case kQ8Tile256x256: return run(Q8DmaTile<F, 256, 256, 2, 128, 2>{});
        case kQ8Tile256x128: return run(Q8DmaTile<F, 256, 128, 4, 128, 3>{});
        case kQ8Tile256x256Rows64: return run(Q8DmaTile<F, 256, 256, 2>{});
        default: return run(Q8DmaTile<F, 256, 128, 4>{});
      }
    });
  const int tiles_m = (M + 127) / 128, tiles_n = (N + 127) / 128;
  const dim3 grid(((tiles_m * tiles_n + 7) / 8) * 8), block(256);
  const size_t lds = 65536;
  auto launch = [&](auto fp8_c) {
    return dispatch_epilogue(mode, "ifx_gemm_q8", [&](auto epi_c) {
      return launch_lds<gemm_q8_kernel<decltype(fp8_c)::value, decltype(epi_c)::value>>(grid, block, lds, s, "ifx_gemm_q8", xp, ldx, wp, y, ldy, M, N, K, tiles_m, tiles_n, ea);
    });
  };
  const int rc = dispatch_q8_format(format, launch);
  if (rc != IFX_OK) return rc;
  return check_launch("ifx_gemm_q8");
}

extern "C" int ifx_gemm_q8(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                           const ifx_bf16* bias, ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K,
                           int32_t format, const ifx_epilogue* epi, void* stream) {
  return gemm_q8_impl(xq, ldx, x_scale, wq, w_scale, bias, y, ldy, M, N, K, format, epi, stream, nullptr, 0);
}

// The plan's ws_bytes for a launch with ideal operands and all the workspace it could ask for — under gemm_variant 0 and 22.  Every other
// variant that leaves the choice to the shape (4 .. 21, 26 .. 29) splits too when it is handed a workspace and the rounds model picks the
// 256-token tile, but its callers have always been told 0, and still are.
extern "C" int64_t ifx_gemm_q8_workspace_bytes(int32_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0 || (gemm_variant() != 0 && gemm_variant() != 22)) return 0;
  GemmRequest r{M, N, K, IFX_EPI_BIAS};
  r.ws_bytes = INT64_MAX;
  return gemm_q8_plan(r, gemm_variant(), gemm_small_split()).ws_bytes;
}

extern "C" int ifx_gemm_q8_ws(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                              const ifx_bf16* bias, ifx_bf16* y, int32_t ldy, int32_t M, int32_t N, int32_t K, int32_t format,
                              const ifx_epilogue* epi, void* workspace, int64_t workspace_bytes, void* stream) {
  return gemm_q8_impl(xq, ldx, x_scale, wq, w_scale, bias, y, ldy, M, N, K, format, epi, stream, nullptr, 0, workspace, workspace_bytes);
}

extern "C" int ifx_gemm_q8_quant_out(const void* xq, int32_t ldx, const float* x_scale, const void* wq, const float* w_scale,
                                     const ifx_bf16* bias, void* yq, int32_t ldyq, int32_t M, int32_t N, int32_t K, int32_t format,
                                     const ifx_epilogue* epi, const float* out_divisor, int32_t via_bf16, void* stream) {
  IFX_REQUIRE(out_divisor && epi && N % 8 == 0, "ifx_gemm_q8_quant_out: out_divisor / epilogue missing or N %% 8 != 0");
  return gemm_q8_impl(xq, ldx, x_scale, wq, w_scale, bias, (ifx_bf16*)yq, ldyq, M, N, K, format, epi, stream, out_divisor, via_bf16);
}

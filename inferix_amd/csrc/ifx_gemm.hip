// bf16 linear layer on MFMA with fused epilogues (gfx950).
//
//   y[M,N] = epilogue( x[M,K] @ W[N,K]^T + bias[N] )
//
// Both operands are K-contiguous (activations token-major, nn.Linear weights
// [out,in]), which is the natural MFMA layout: every lane's 8-element fragment is one
// 16-byte load.  The kernel computes the TRANSPOSED tile D = W_tile · x_tile^T
// (A-operand = W rows, B-operand = x rows) so that each lane ends up with 4
// CONSECUTIVE output channels of one token: bias / gate / residual / store are
// 8-byte vector accesses along the contiguous dimension.
//
// Tiling (v1): 128(tokens) x 128(channels) x 64(K) per workgroup, 4 waves (2x2),
// each wave 64x64 = 4x4 fragments of v_mfma_f32_16x16x32_bf16; operands staged
// global -> registers -> LDS (double buffered, one barrier per K-tile, loads for
// tile t+1 issued before the MFMAs of tile t); LDS rows are 128 B with the 16-byte
// chunk index XOR-swizzled by (row & 7) so ds_read_b128 fragment reads are
// bank-conflict free.  64 KiB LDS -> 2 workgroups per CU.
#include "ifx_gemm_tile.h"

namespace ifx {

constexpr int BM = 128, BN = 128, BK = 64;

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const unsigned short* __restrict__ x, int ldx,
                                                           const unsigned short* __restrict__ w,
                                                           unsigned short* __restrict__ y, int ldy, int M, int N,
                                                           int K, int tiles_m, int tiles_n, EpiArgs ea) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // [buf][X|W][128 rows][128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  // XCD-aware grouped raster (ifx_gemm_tile.h): XCD (bid & 7) owns a contiguous id range; ids walk
  // GM token-tiles then the next channel-tile, so co-resident workgroups share operand panels in L2.
  const int total = tiles_m * tiles_n, per_xcd = (total + 7) / 8;
  const int t_id = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per_xcd || t_id >= total) return;
  const TileOrigin org = tile_origin_of<BM, BN, 8>(t_id, tiles_m, tiles_n);
  const int m_base = org.m, n_base = org.n;

  // staging assignment: 4 chunks of 16 B per matrix per thread
  const unsigned short* gx[4];
  const unsigned short* gw[4];
  int lds_off[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int q = tid + 256 * p, row = q >> 3, c = q & 7;
    const int mr = min(m_base + row, M - 1), nr = min(n_base + row, N - 1);
    gx[p] = x + (size_t)mr * ldx + c * 8;
    gw[p] = w + (size_t)nr * K + c * 8;
    lds_off[p] = row * 128 + ((c ^ (row & 7)) << 4);
  }
  u32x4 rx[4], rw[4];
  auto gload = [&](int kt) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      rx[p] = *reinterpret_cast<const u32x4*>(gx[p] + (size_t)kt * BK);
      rw[p] = *reinterpret_cast<const u32x4*>(gw[p] + (size_t)kt * BK);
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

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = K / BK;
  gload(0);
  lstore(0);
  __syncthreads();

  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) gload(kt + 1);
    const unsigned char* bx = smem + buf * 32768;
    const unsigned char* bw = bx + 16384;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[4], b[4];
      const int c = ks * 4 + fq;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wn * 64 + i * 16 + fr;
        a[i] = *reinterpret_cast<const bf16x8*>(bw + row * 128 + ((c ^ (row & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wm * 64 + j * 16 + fr;
        b[j] = *reinterpret_cast<const bf16x8*>(bx + row * 128 + ((c ^ (row & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < KT) lstore(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds D[n = n0+16i+4*fq+{0..3}][m = m0+16j+fr]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m_base + wm * 64 + j * 16 + fr;
    if (m >= M) continue;
    const unsigned short* gate_row = nullptr;
    if (EPI == IFX_EPI_GATE_RES)
      gate_row = ea.mod + ((size_t)(m / ea.rows_per_group) * ea.mod_slots + ea.gate_slot) * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n_base + wn * 64 + i * 16 + fq * 4;
      if (n >= N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
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
      *reinterpret_cast<u16x4*>(y + (size_t)m * ldy + n) = o;
    }
  }
}

}  // namespace ifx

using namespace ifx;

// ifx_gemm_bf16 is this with no workspace.  Check the arguments, say what the call is (GemmRequest), let gemm_plan of ifx_gemm_plan.h decide, launch what it decided.  The meaning
// of every gemm_variant is the table kGemmVariants there.
extern "C" int ifx_gemm_bf16_ws(const ifx_bf16* x, int32_t ldx, const ifx_bf16* w, const ifx_bf16* bias, ifx_bf16* y,
                                int32_t ldy, int32_t M, int32_t N, int32_t K, const ifx_epilogue* epi, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  IFX_REQUIRE(x && w && y && M >= 0 && N > 0 && K > 0, "ifx_gemm_bf16: null/empty operand");
  IFX_REQUIRE(K % BK == 0, "ifx_gemm_bf16: K (%d) must be a multiple of %d", K, BK);   // 64; also covers the 32-deep tiles
  IFX_REQUIRE(N % 4 == 0 && ldx % 8 == 0 && ldy % 4 == 0, "ifx_gemm_bf16: N %% 4, ldx %% 8, ldy %% 4 required");
  int mode;
  EpiArgsP ea;
  if (const int rc = resolve_epilogue(epi, bias, "ifx_gemm_bf16", &mode, &ea)) return rc;
  // base alignment: every kernel of the family reads x and W in 16-byte chunks; bias, residual, gate rows and y are touched in 8-byte
  // vectors by the register-staged kernel and in 16-byte vectors (bias: 8) by all the others
  IFX_REQUIRE(!(((uintptr_t)x | (uintptr_t)w) & 15), "ifx_gemm_bf16: x and w must be 16-byte aligned");
  IFX_REQUIRE(!(((uintptr_t)y | (uintptr_t)bias | (uintptr_t)ea.residual | (uintptr_t)ea.mod) & 7),
              "ifx_gemm_bf16: y, bias, residual and mod must be 8-byte aligned");
  if (M == 0) return IFX_OK;
  GemmRequest r = gemm_request(M, N, K, mode, ea, y, ldy, workspace, workspace_bytes);
  r.y2 = epi != nullptr && epi->y2 != nullptr;
  const GemmPlan plan = gemm_plan(r, gemm_variant(), gemm_small_split());
  IFX_REQUIRE(plan.path != kGemmPathRefuseY2,
              "ifx_gemm_bf16: the second destination (y2) needs the bias epilogue, N %% 64 == 0, 8-byte aligned bias and the ping-pong tiles");
  hipStream_t s = (hipStream_t)stream;
  void* const ws = plan.ws_bytes > 0 ? workspace : nullptr;
  switch (plan.path) {
    case kGemmPathW4: return launch_gemm_w4(x, ldx, w, y, ldy, M, N, K, mode, ea, s, plan.ks, ws);
    case kGemmPathPp:
      if (plan.y2) ea.y2 = epi->y2, ea.ldy2 = epi->ldy2, ea.split_col = epi->split_col;
      return launch_gemm_pp(x, ldx, w, y, ldy, M, N, K, mode, ea, s, plan.tj, plan.ks, ws);
    case kGemmPathLdsDma: return launch_gemm_lds_dma(plan.tile, x, ldx, w, y, ldy, M, N, K, mode, ea, s);
    default: break;      // kGemmPathRegStaged: this file's kernel
  }
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const dim3 grid(((tiles_m * tiles_n + 7) / 8) * 8), block(256);
  const size_t lds = 65536;
  const int rc = dispatch_epilogue(mode, "ifx_gemm_bf16", [&](auto epi_c) {
    return launch_lds<gemm_bf16_kernel<decltype(epi_c)::value>>(grid, block, lds, s, "ifx_gemm_bf16", x, ldx, w, y, ldy, M, N, K, tiles_m, tiles_n, ea);
  });
  if (rc != IFX_OK) return rc;
  return check_launch("ifx_gemm_bf16");
}

extern "C" int ifx_gemm_bf16(const ifx_bf16* x, int32_t ldx, const ifx_bf16* w, const ifx_bf16* bias, ifx_bf16* y,
                             int32_t ldy, int32_t M, int32_t N, int32_t K, const ifx_epilogue* epi, void* stream) {
  return ifx_gemm_bf16_ws(x, ldx, w, bias, y, ldy, M, N, K, epi, nullptr, 0, stream);
}

// The plan's ws_bytes for a launch with ideal operands and all the workspace it could ask for.  Three groups of forced variants have
// always been told MORE than their launches touch, and still are (callers may size buffers by it):
//   22, 23   : the two-workgroup split's bytes for every (N, K) of gemm_pp_split — also for an N the ping-pong tile then refuses
//              (N % 64 != 0) and for a 192-token tiling of more than 1024 tiles, which runs unsplit;
//   26       : the stream-K slots also below the 48 K-step units at which the launch takes stream-K;
//   27 .. 29 : the partial slots also beyond the 1024 the flag page covers (such a launch falls to the 64 x 64 tile).
extern "C" int64_t ifx_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const GemmVariant v = gemm_variant_row(gemm_variant());
  const bool mult64 = N % 64 == 0 && K % 64 == 0;
  if (v.kind == kGemmPp && v.takes_ws) return (int64_t)gemm_pp_workspace_bytes(M, N, K);
  if (v.kind == kGemmPpStreamK) return mult64 ? (int64_t)gemm_pp_stream_k_workspace_bytes() : 0;
  if (v.kind == kGemmPpKParts) return mult64 && (K / 64) % v.ks == 0 ? (int64_t)gemm_pp_small_workspace_bytes(M, N, v.ks) : 0;
  GemmRequest r{M, N, K, IFX_EPI_BIAS};
  r.ws_bytes = INT64_MAX;
  return gemm_plan(r, gemm_variant(), gemm_small_split()).ws_bytes;
}

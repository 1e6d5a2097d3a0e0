// fp32 T5 v1.1 caption-encoder kernels (MAGI-1 `T5Embedder`), gfx950 only.  Every operand and result is fp32: upstream
// runs HuggingFace's `T5EncoderModel` with torch_dtype=torch.float (inferix/pipeline/magi/prompt_process.py:135-144), so these
// kernels keep fp32 arithmetic end to end and parity is checked at the 1e-6 level (no bf16 rounding anywhere in the chain).
//
//   ifx_gemm_f32           nn.Linear (no bias) of T5Attention q/k/v/o and T5DenseGatedActDense wi_0/wi_1/wo, + the residual add of
//                          T5LayerSelfAttention / T5LayerFF.  v_mfma_f32_32x32x2_f32, operands through LDS, ONE accumulation chain per
//                          output element in k order 0 .. K-1 (the instruction is a k-ordered fmaf chain): a row's result depends
//                          neither on M nor on the tile height that ran.
//   ifx_t5_attention_f32   T5Attention between its q/k/v and o linears: s = q.k + bias[h][key - query], key-padding mask, fp32
//                          softmax, p.v.  Key tiles of 32 with an online softmax (fp32 K and V of a head at 800 keys are 400 KiB).
//   ifx_rmsnorm_f32        T5LayerNorm.
//   ifx_t5_gated_gelu_f32  NewGELUActivation(wi_0 x) * (wi_1 x) of T5DenseGatedActDense.
#include "ifx_launch.h"

namespace ifx {
namespace t5f {

typedef __attribute__((ext_vector_type(4))) float f4;

// ---- GEMM ---------------------------------------------------------------------------------------------------------------------
constexpr int BK = 32;
constexpr int LDT = BK + 1;      // LDS row pitch in floats: a fragment read is one fp32 per lane with lanes along the rows, so the pitch
                                 // must be odd for the 32 lanes of a half wave to fall on 32 banks (a pitch of BK is a 32-way conflict)

struct GemmArgs {
  const float* x;
  const float* w;
  const float* res;
  float* y;
  int ldx, ld_res, ldy;
  int M, N, K;
};

// Block tile BM x BN, WM x WN waves, each wave a (BM / WM) x (BN / WN) tile as TM x TN accumulators of 32 x 32.
// A = x rows (lane l: A[i = l & 31][k = l >> 5]), B = w rows (B[k = l >> 5][j = l & 31] = w[j][k]); D column = lane & 31 (output
// column), D row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void gemm_f32_kernel(GemmArgs A) {
  constexpr int NT = 64 * WM * WN;
  constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
  constexpr int XV = BM * (BK / 4) / NT, WV = BN * (BK / 4) / NT;      // float4 per thread per K step
  static_assert(BM * (BK / 4) % NT == 0 && BN * (BK / 4) % NT == 0, "staging loops need whole passes");
  __shared__ float Xs[BM * LDT];
  __shared__ float Ws[BN * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
  const int wrow = wm * (BM / WM), wcol = wn * (BN / WN);
  const bool wave_live = col0 + wcol < A.N;      // N % 64 == 0 and a wave's columns start on a multiple of 32 inside a 64 block

  f4 xr[XV], wr[WV];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int idx = tid + i * NT, r = idx >> 3, c = idx & 7;
      const int row = row0 + r;
      xr[i] = row < A.M ? *reinterpret_cast<const f4*>(A.x + (size_t)row * A.ldx + k0 + c * 4) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      const int idx = tid + i * NT, r = idx >> 3, c = idx & 7;
      const int col = col0 + r;
      wr[i] = col < A.N ? *reinterpret_cast<const f4*>(A.w + (size_t)col * A.K + k0 + c * 4) : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int idx = tid + i * NT, r = idx >> 3, c = idx & 7;
#pragma unroll
      for (int e = 0; e < 4; ++e) Xs[r * LDT + c * 4 + e] = xr[i][e];
    }
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      const int idx = tid + i * NT, r = idx >> 3, c = idx & 7;
#pragma unroll
      for (int e = 0; e < 4; ++e) Ws[r * LDT + c * 4 + e] = wr[i][e];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  fetch(0);
  stage();
  __syncthreads();
  for (int k0 = 0; k0 < A.K; k0 += BK) {
    const bool more = k0 + BK < A.K;
    if (more) fetch(k0 + BK);
    if (wave_live) {
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {
        float a[TM], b[TN];
#pragma unroll
        for (int m = 0; m < TM; ++m) a[m] = Xs[(wrow + m * 32 + l31) * LDT + kk * 2 + hi];
#pragma unroll
        for (int n = 0; n < TN; ++n) b[n] = Ws[(wcol + n * 32 + l31) * LDT + kk * 2 + hi];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
      }
    }
    __syncthreads();
    if (more) {
      stage();
      __syncthreads();
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      const int col = col0 + wcol + n * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + wrow + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (row < A.M) {
          float v = acc[m][n][r];
          if (A.res) v += A.res[(size_t)row * A.ld_res + col];
          A.y[(size_t)row * A.ldy + col] = v;
        }
      }
    }
}

// ---- attention ----------------------------------------------------------------------------------------------------------------
constexpr int HD = 64;
constexpr int KP = HD + 1;       // K tile pitch: the S^T = K Q^T operand is read with lanes along the keys (odd pitch, as above)

struct AttnArgs {
  const float* q;
  const float* k;
  const float* v;
  float* out;
  const float* bias;               // [heads][2L-1]: bias of relative offset (key - query) + L - 1
  const int* seq_lens;             // [batch] valid keys per prompt (device)
  int ldq, ldk, ldv, ldo;
  int L, heads, q_tiles, query_rows;
};

// exp(arg) for arg <= 0 as exp2(a) (1 + r ln 2), a + r = arg log2(e) carried in two floats: v_exp_f32 on the rounded product alone
// would lose |arg| 2^-24 of relative accuracy
__device__ __forceinline__ float exp_neg(float arg) {
  const float a = arg * 1.4426950408889634f;
  float r = fmaf(arg, 1.4426950408889634f, -a);
  r = fmaf(arg, 1.9259629911266175e-8f, r);
  return __builtin_amdgcn_exp2f(a) * fmaf(r, 0.6931471805599453f, 1.0f);
}

// One workgroup = 4 waves x 32 queries of one (prompt, head).  Per 32-key tile (K and V staged in LDS, shared by the 4 waves):
//   S^T = K Q^T with 32 MFMA 32x32x2 (keys in the accumulator registers, the lane's own query in its column);
//   online softmax per lane (the lane and lane ^ 32 hold the two halves of the keys of one query: one exchange per tile);
//   O^T += V^T P^T with P fed straight from the accumulators: the k slot (lane >> 5) of MFMA step (a, b) is relabelled to the key
//   8a + 4 (lane >> 5) + b that accumulator register 4a + b holds, and V is read from LDS in that same order.
__global__ __launch_bounds__(256) void t5_attention_f32_kernel(AttnArgs A) {
  __shared__ float Ks[32 * KP];
  __shared__ float Vs[32 * HD];
  __shared__ float bt[2 * 1024];
  const int L = A.L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  int rem = blockIdx.x;
  const int qt = rem % A.q_tiles;
  rem /= A.q_tiles;
  const int h = rem % A.heads, b = rem / A.heads;
  const int seq = min(max(A.seq_lens[b], 0), L);
  const size_t row0 = (size_t)b * L;
  const int q = qt * 128 + wave * 32 + l31;
  const int q_end = A.query_rows ? seq : L;      // rows the caller wants computed; the others (< L) get zeros
  const bool q_live = q < q_end;
  float* op = A.out + (row0 + q) * A.ldo + h * HD;

  if (qt * 128 >= q_end || seq == 0) {           // nothing to compute in this workgroup (uniform): zeros, no key is read
    if (q < L) {
#pragma unroll
      for (int c = 0; c < HD / 8; ++c) *reinterpret_cast<f4*>(op + c * 8 + hi * 4) = f4{0.f, 0.f, 0.f, 0.f};
      // the two lanes of a query cover columns {8c + 4hi .. + 3}: all 64
    }
    return;
  }

  for (int i = tid; i < 2 * L - 1; i += 256) bt[i] = A.bias[(size_t)h * (2 * L - 1) + i];

  // Q^T operand: qf[s] = Q[query][2 s + hi]; a query past q_end contributes zeros (its row may hold anything, NaN included)
  float qf[32];
  {
    const float* qp = A.q + (row0 + min(q, L - 1)) * A.ldq + h * HD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const f4 t = q_live ? *reinterpret_cast<const f4*>(qp + i * 4) : f4{0.f, 0.f, 0.f, 0.f};
      qf[2 * i] = hi ? t[1] : t[0];
      qf[2 * i + 1] = hi ? t[3] : t[2];
    }
  }
  const int qc = min(q, L - 1);

  f32x16 o[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[hb][r] = 0.f;
  float m = -1e30f, l = 0.f;

  const int ntiles = (seq + 31) / 32;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();      // the previous tile's reads are done (first pass: bt is written)
    for (int idx = tid; idx < 32 * 16; idx += 256) {
      const int key = idx >> 4, c = idx & 15;
      const int gk = kt * 32 + key;
      f4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (gk < seq) {      // keys past the valid length are never read
        kv = *reinterpret_cast<const f4*>(A.k + (row0 + gk) * A.ldk + h * HD + c * 4);
        vv = *reinterpret_cast<const f4*>(A.v + (row0 + gk) * A.ldv + h * HD + c * 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) Ks[key * KP + c * 4 + e] = kv[e];
      *reinterpret_cast<f4*>(Vs + key * HD + c * 4) = vv;
    }
    __syncthreads();

    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int st = 0; st < 32; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31 * KP + st * 2 + hi], qf[st], s, 0, 0, 0);

    float tm = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
      const bool valid = key < seq;
      s[r] = valid ? s[r] + bt[key - qc + L - 1] : -1e30f;
      tm = fmaxf(tm, s[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);               // finite from the first tile on: key 0 is valid
    const float alpha = exp_neg(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
      s[r] = key < seq ? exp_neg(s[r] - mn) : 0.f;      // a masked key has probability exactly 0
      ps += s[r];
    }
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[hb][r] *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = (r >> 2) * 8 + hi * 4 + (r & 3);
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
        o[hb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * HD + hb * 32 + l31], s[r], o[hb], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 32, 64);
  if (q >= L) return;
  const float inv = q_live ? 1.0f / l : 0.f;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = q_live ? o[hb][4 * g + e] * inv : 0.f;
      *reinterpret_cast<f4*>(op + hb * 32 + g * 8 + hi * 4) = ov;
    }
}

// ---- row kernels --------------------------------------------------------------------------------------------------------------
// T5LayerNorm: w * (x * rsqrt(mean(x^2) + eps)); one wave per row, 4 rows per workgroup
__global__ __launch_bounds__(256) void rmsnorm_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, float* y,
                                                           int ldy, int rows, int dim, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xp = x + (size_t)row * ldx;
  float* yp = y + (size_t)row * ldy;
  float ss = 0.f;
  for (int c = lane; c < dim; c += 64) {
    const float v = xp[c];
    ss = fmaf(v, v, ss);
  }
  const float var = wave_sum(ss) / (float)dim;
  const float rs = 1.0f / sqrtf(var + eps);
  for (int c = lane; c < dim; c += 64) yp[c] = w[c] * (xp[c] * rs);
}

// h = gelu_new(g) * u, gelu_new(g) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3))); gu = [rows][2 f] = (g | u)
__global__ __launch_bounds__(256) void gated_gelu_f32_kernel(const float* __restrict__ gu, float* __restrict__ h, long long total4,
                                                              int f4n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long row = i / f4n;
  const int c = (int)(i - row * f4n);
  const f4 g = *reinterpret_cast<const f4*>(gu + (row * 2 * f4n + c) * 4);
  const f4 u = *reinterpret_cast<const f4*>(gu + (row * 2 * f4n + f4n + c) * 4);
  f4 ov;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = g[e];
    const float inner = 0.7978845608028654f * (t + 0.044715f * (t * t * t));
    ov[e] = (0.5f * t * (1.0f + tanhf(inner))) * u[e];
  }
  *reinterpret_cast<f4*>(h + i * 4) = ov;
}

}  // namespace t5f
}  // namespace ifx

using namespace ifx;

#define IFX_UNSUP(cond, ...)       \
  do {                             \
    if (!(cond)) {                 \
      ifx::set_error(__VA_ARGS__); \
      return IFX_EUNSUP;           \
    }                              \
  } while (0)

extern "C" int ifx_gemm_f32(const float* x, int32_t ldx, const float* w, const float* res, int32_t ld_res, float* y, int32_t ldy,
                            int32_t M, int32_t N, int32_t K, int32_t tile, void* stream) {
  IFX_REQUIRE(x && w && y, "ifx_gemm_f32: null argument");
  IFX_REQUIRE(M >= 1 && N >= 1 && K >= 1, "ifx_gemm_f32: empty shape %d x %d x %d", M, N, K);
  IFX_REQUIRE(tile >= 0 && tile <= 2, "ifx_gemm_f32: tile %d (0 by M, 1 the 128-row tile, 2 the 32-row tile)", tile);
  IFX_UNSUP(K % 64 == 0 && N % 64 == 0, "ifx_gemm_f32: built for K %% 64 == 0 and N %% 64 == 0, got N %d K %d", N, K);
  IFX_UNSUP(ldx % 4 == 0 && ldx >= K && ldy >= N && (!res || ld_res >= N), "ifx_gemm_f32: row strides (x %d, y %d, res %d) must cover "
            "the rows, x in 16-byte steps", ldx, ldy, ld_res);
  IFX_UNSUP((((uintptr_t)x | (uintptr_t)w) & 15) == 0 && (((uintptr_t)y | (uintptr_t)res) & 3) == 0,
            "ifx_gemm_f32: x and w must be 16-byte aligned");
  t5f::GemmArgs a{x, w, res, y, ldx, ld_res, ldy, M, N, K};
  // the 128-row tile when it alone fills the chip (800 x 4096: 7 x 32 tiles on 256 CUs), else the 32-row tile (120 x 4096: 4 x 64)
  const bool tall = tile ? tile == 1 : (long long)((M + 127) / 128) * ((N + 127) / 128) >= device_cu_count() / 2;
  if (tall)
    hipLaunchKernelGGL((t5f::gemm_f32_kernel<128, 128, 2, 2>), dim3((N + 127) / 128, (M + 127) / 128), dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((t5f::gemm_f32_kernel<32, 64, 1, 2>), dim3(N / 64, (M + 31) / 32), dim3(128), 0, (hipStream_t)stream, a);
  return check_launch("ifx_gemm_f32");
}

extern "C" int ifx_t5_attention_f32(const float* q, int32_t ldq, const float* k, int32_t ldk, const float* v, int32_t ldv, float* out,
                                    int32_t ldo, const float* rel_bias, const int32_t* seq_lens, int32_t batch, int32_t seq_len_padded,
                                    int32_t heads, int32_t query_rows, void* stream) {
  IFX_REQUIRE(q && k && v && out && rel_bias && seq_lens, "ifx_t5_attention_f32: null argument");
  IFX_REQUIRE(batch >= 1 && heads >= 1, "ifx_t5_attention_f32: empty batch / heads");
  IFX_REQUIRE(query_rows == 0 || query_rows == 1, "ifx_t5_attention_f32: query_rows %d (0 every padded row, 1 valid rows)", query_rows);
  IFX_REQUIRE(seq_len_padded >= 8 && seq_len_padded <= 1024 && seq_len_padded % 8 == 0,
              "ifx_t5_attention_f32: padded length %d not a multiple of 8 in [8, 1024]", seq_len_padded);
  IFX_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ldq >= heads * 64 && ldk >= heads * 64 &&
              ldv >= heads * 64 && ldo >= heads * 64, "ifx_t5_attention_f32: row strides must be multiples of 4 covering heads x 64");
  IFX_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "ifx_t5_attention_f32: q, k, v, out must be 16-byte aligned");
  t5f::AttnArgs a;
  a.q = q;
  a.k = k;
  a.v = v;
  a.out = out;
  a.bias = rel_bias;
  a.seq_lens = seq_lens;
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.ldo = ldo;
  a.L = seq_len_padded;
  a.heads = heads;
  a.q_tiles = (seq_len_padded + 127) / 128;
  a.query_rows = query_rows;
  hipLaunchKernelGGL(t5f::t5_attention_f32_kernel, dim3(batch * heads * a.q_tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_t5_attention_f32");
}

extern "C" int ifx_rmsnorm_f32(const float* x, int32_t ldx, const float* w, float* y, int32_t ldy, int32_t rows, int32_t dim, float eps,
                               void* stream) {
  IFX_REQUIRE(x && w && y && rows >= 0 && ldx >= dim && ldy >= dim, "ifx_rmsnorm_f32: bad arguments");
  IFX_UNSUP(dim >= 64 && dim <= 4096 && dim % 64 == 0, "ifx_rmsnorm_f32: built for widths that are multiples of 64 up to 4096, got %d", dim);
  if (rows == 0) return IFX_OK;
  hipLaunchKernelGGL(t5f::rmsnorm_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, w, y, ldy, rows, dim, eps);
  return check_launch("ifx_rmsnorm_f32");
}

extern "C" int ifx_t5_gated_gelu_f32(const float* gate_up, float* h, int32_t rows, int32_t ffn, void* stream) {
  IFX_REQUIRE(gate_up && h && rows >= 0 && ffn > 0 && ffn % 4 == 0, "ifx_t5_gated_gelu_f32: bad arguments (ffn %d)", ffn);
  IFX_REQUIRE((((uintptr_t)gate_up | (uintptr_t)h) & 15) == 0, "ifx_t5_gated_gelu_f32: gate_up and h must be 16-byte aligned");
  if (rows == 0) return IFX_OK;
  const long long total4 = (long long)rows * (ffn / 4);
  hipLaunchKernelGGL(t5f::gated_gelu_f32_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gate_up, h,
                     total4, ffn / 4);
  return check_launch("ifx_t5_gated_gelu_f32");
}

// MAGI ViT-VAE tile decoder kernels (BASELINE config 5, PER_BLOCK decode), gfx950 only: the three pieces of `ViTDecoder`
// (inferix/models/magi/vae/vae_module.py:569-716) that are not a LayerNorm or a linear.
//
//   vit_head_prep_kernel     `Attention.forward` :281-292 on the fused qkv GEMM output, in place: `ManualLayerNorm` (:229-242) per
//                            (token, q | k | v, head) in the reference's bf16 op chain, then the interleaved rotation (:142-150) of q and
//                            k for the tokens behind the class token.  One 8-lane group per 64-channel head, 16-byte accesses.
//   vit_attention_kernel     softmax(q k^T / 8) v, non-causal, head_dim 64, any key count.  Flash style: a workgroup is 4 waves x 32
//                            queries; 64-key tiles of K (16-byte chunks XOR-swizzled by key & 7) and V^T go through two LDS buffers by a
//                            register-staged loader (the next tile's global loads are in flight while this one is multiplied; one
//                            barrier per tile).  Both products are MFMA 32x32x16 bf16 in the transposed form of t5_attention_kernel
//                            (ifx_t5.hip): S^T = K Q^T puts keys in registers and the query in the lane, so the probabilities feed the
//                            P operand of O^T = V^T P^T straight from the accumulators.  fp32 online softmax in the exp2 domain; the
//                            two lanes (l, l + 32) that share a query exchange their tile maximum once per tile.  Keys past `tokens`
//                            are never read (their LDS rows are zero) and are masked to -inf before the row maximum; query rows past
//                            `tokens` are never stored.  Every loop bound is a function of the launch arguments.
//   vit_unpatch_conv_kernel  `ViTDecoder.forward` :712-715: the patch rearrangement + zero-padded 3x3x3 Conv3d(4 -> 3) in one pass.  One
//                            thread per output pixel, the token-major rows indexed directly, weights as fp32 in LDS, fp32 accumulate,
//                            one rounding.
//   vit_tile_blend_kernel    `TileProcessor.tiled_decode` (inferix/distributed/parallelism/tile_parallel.py:412-448) behind the tile
//                            decodes, in one pass over the output: every output pixel finds the tile that owns it, loads that tile's
//                            value and applies the temporal, the vertical and the horizontal blend against the RAW neighbour tiles
//                            in the reference's eager bf16 chain, bf16(bf16(a w1) + bf16(b w2)); the weights w1 = fp32(1.0 - p / e')
//                            and w2 = fp32(p / e') (quotient and difference in double) come from the descriptor table, where the
//                            host put them as the reference's Python floats give them.  The crop and the concatenation are the
//                            output index, the uint8 tail of `VaeHelper.decode` is a second store.  One lane owns 8 consecutive
//                            pixels of a row (16-byte accesses) when every x extent is a multiple of 8, one pixel otherwise; the
//                            grid is (row units, frame, sample x channel), so a lane divides one 32-bit number once.
#include "ifx_common.h"

namespace ifx {
namespace vit {

constexpr int HD = 64;

// ---------------------------------------------------------------------------------------------------------------------------------
struct PrepArgs {
  unsigned short* qkv;             // [rows, 3 * heads * 64], row stride ld
  const unsigned short* sin_t;     // [tokens - cls, 64]
  const unsigned short* cos_t;
  long long units;                 // rows * 3 * heads
  int ld, tokens, heads, cls, do_norm, do_rope;
  float eps;
};

// sum over the 8 lanes of a head group (quad xor 1, xor 2, then the mirror inside the half row: lane i + lane 7 - i)
__device__ __forceinline__ float group8_sum(float v) {
  v += dpp_or<0xB1, 0xf>(0.f, v);
  v += dpp_or<0x4E, 0xf>(0.f, v);
  v += dpp_or<0x141, 0xf>(0.f, v);
  return v;
}

__global__ __launch_bounds__(256) void vit_head_prep_kernel(PrepArgs A) {
  const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int l8 = threadIdx.x & 7;
  const bool live = g < A.units;
  const long long u = live ? g : A.units - 1;           // a valid address for the lanes behind the end; they store nothing
  const int per_row = 3 * A.heads;
  const long long row = u / per_row;
  const int rem = (int)(u - row * per_row);             // part * heads + head
  const int part = rem / A.heads;
  unsigned short* p = A.qkv + row * A.ld + rem * HD + l8 * 8;
  const u16x8 raw = *reinterpret_cast<const u16x8*>(p);
  const int tok = (int)(row % A.tokens);
  const bool rotate = A.do_rope && part < 2 && tok >= A.cls;
  u16x8 sv = raw, cv = raw;
  if (rotate) {
    sv = *reinterpret_cast<const u16x8*>(A.sin_t + (size_t)(tok - A.cls) * HD + l8 * 8);
    cv = *reinterpret_cast<const u16x8*>(A.cos_t + (size_t)(tok - A.cls) * HD + l8 * 8);
  }
  float x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = bf2f(raw[i]);
  if (A.do_norm) {
    // ManualLayerNorm on a bf16 tensor: mean and population std come out of fp32 reductions as bf16 values; the difference, the sum
    // with eps and the quotient are bf16 operations (each rounded)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += x[i];
    const float mean_f = group8_sum(s) * (1.0f / HD);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = x[i] - mean_f;
      ss += d * d;
    }
    const float std_b = rbf(sqrtf(group8_sum(ss) * (1.0f / HD)));
    const float mean_b = rbf(mean_f);
    const float den = rbf(std_b + A.eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = rbf(rbf(x[i] - mean_b) / den);
  }
  if (rotate) {
    // x cos + rot(x) sin with rot(x)[2i] = -x[2i+1], rot(x)[2i+1] = x[2i]; both products and the sum rounded to bf16
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      const float a = x[i], b = x[i + 1];
      x[i] = rbf(rbf(a * bf2f(cv[i])) + rbf(-b * bf2f(sv[i])));
      x[i + 1] = rbf(rbf(b * bf2f(cv[i + 1])) + rbf(a * bf2f(sv[i + 1])));
    }
  }
  u16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(x[i]);
  if (live) *reinterpret_cast<u16x8*>(p) = o;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct AttnArgs {
  const unsigned short* q;
  const unsigned short* k;
  const unsigned short* v;
  unsigned short* out;
  int ldq, ldk, ldv, ldo;          // row strides (elements)
  int tokens, heads, q_tiles;
};

constexpr int KT = 64;                       // keys per tile
constexpr int VPB = KT * 2 + 8;              // V^T row pitch in bytes (bank spread for the 8-byte reads)
constexpr int KS_BYTES = KT * 128;           // [64 keys][64 ch] bf16
constexpr int BUF_BYTES = KS_BYTES + HD * VPB;

__global__ __launch_bounds__(256) void vit_attention_kernel(AttnArgs A) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  int rem = blockIdx.x;
  const int qt = rem % A.q_tiles;
  rem /= A.q_tiles;
  const int h = rem % A.heads, b = rem / A.heads;
  const int T = A.tokens;
  const size_t row0 = (size_t)b * T;
  const int nt = (T + KT - 1) / KT;

  // loader: thread -> chunks (key, c) = (tid >> 3 (+ 32), tid & 7) of K and of V; rows past the end are zeros, never read
  const int lk = tid >> 3, lc = tid & 7;
  u16x8 kr[2], vr[2];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = t * KT + lk + i * 32;
      const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      kr[i] = z;
      vr[i] = z;
      if (key < T) {
        kr[i] = *reinterpret_cast<const u16x8*>(A.k + (row0 + key) * A.ldk + h * HD + lc * 8);
        vr[i] = *reinterpret_cast<const u16x8*>(A.v + (row0 + key) * A.ldv + h * HD + lc * 8);
      }
    }
  };
  auto store_tile = [&](int buf) {
    unsigned char* Ks = smem + buf * BUF_BYTES;
    unsigned char* Vt = Ks + KS_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = lk + i * 32;
      *reinterpret_cast<u16x8*>(Ks + key * 128 + ((lc ^ (key & 7)) << 4)) = kr[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) *reinterpret_cast<unsigned short*>(Vt + (lc * 8 + e) * VPB + key * 2) = vr[i][e];
    }
  };

  const int q = qt * 128 + wave * 32 + l31;
  const int qc = min(q, T - 1);
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8*>(A.q + (row0 + qc) * A.ldq + h * HD + ks * 16 + hi * 8);

  f32x16 o[2];
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[hb][r] = 0.f;
  float m = -INFINITY, l = 0.f;                                // m in the exp2 domain; l: this lane's half of the keys
  const float sl2 = 0.125f * 1.4426950408889634f;              // 1 / sqrt(64) * log2(e)

  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;
    if (more) load_tile(t + 1);
    const unsigned char* Ks = smem + (t & 1) * BUF_BYTES;
    const unsigned char* Vt = Ks + KS_BYTES;
    // S^T: s[kb][r] is key t*64 + kb*32 + (r/4)*8 + hi*4 + r%4 against this lane's query
    float s[2][16];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int key = kb * 32 + l31;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(Ks + key * 128 + (((ks * 2 + hi) ^ (key & 7)) << 4));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = acc[r] * sl2;
    }
    if (!more) {                                               // the ragged tile: keys past the end leave the maximum and the sum
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = t * KT + kb * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
          if (kk >= T) s[kb][r] = -INFINITY;
        }
    }
    float bm = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) bm = fmaxf(bm, s[kb][r]);
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));                    // both lanes of a query scale the shared accumulators alike
    const float mn = fmaxf(m, bm);                             // finite from tile 0 on: key 0 is always valid
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    unsigned short p[2][16];
    float ps = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(s[kb][r] - mn);
        ps += e;
        p[kb][r] = f2bf(e);
      }
    l = l * alpha + ps;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[hb][r] *= alpha;
    // O^T += V^T P^T: contraction slots 0..3 of a lane are keys k0.., slots 4..7 keys k0 + 8.. (where its accumulators sit)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        u16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = p[kb][(2 * s2 + (j >> 2)) * 4 + (j & 3)];
        const int k0 = kb * 32 + (2 * s2) * 8 + hi * 4;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          const unsigned char* vrow = Vt + (hb * 32 + l31) * VPB;
          const u16x4 a0 = *reinterpret_cast<const u16x4*>(vrow + k0 * 2);
          const u16x4 a1 = *reinterpret_cast<const u16x4*>(vrow + (k0 + 8) * 2);
          const u16x8 av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
          o[hb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, pb), o[hb], 0, 0, 0);
        }
      }
    if (more) store_tile((t + 1) & 1);
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  if (q >= T) return;
  const float inv_l = 1.0f / l;
  unsigned short* op = A.out + (row0 + q) * A.ldo + h * HD;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u16x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = f2bf(o[hb][4 * g + e] * inv_l);
      *reinterpret_cast<u16x4*>(op + hb * 32 + g * 8 + hi * 4) = ov;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct ConvArgs {
  const unsigned short* x;         // [batch * tile_rows, pT*pH*pW*4], row stride ldx; the first `cls` rows of a tile are skipped
  const unsigned short* w;         // [3][4][3][3][3] bf16 (Conv3d weight)
  const unsigned short* bias;      // [3] bf16
  unsigned short* y;               // [batch, 3, T, H, W]
  long long pixels;                // batch * T * H * W
  int ldx, tile_rows, cls;
  int T, H, W, pT, pH, pW;
};

__global__ __launch_bounds__(256) void vit_unpatch_conv_kernel(ConvArgs A) {
  __shared__ float wsm[27 * 4 * 3 + 3];                        // [tap][cin][cout], then the bias
  for (int i = threadIdx.x; i < 27 * 4 * 3; i += 256) {
    const int co = i % 3, ci = (i / 3) & 3, tap = i / 12;
    wsm[i] = bf2f(A.w[(co * 4 + ci) * 27 + tap]);
  }
  if (threadIdx.x < 3) wsm[324 + threadIdx.x] = bf2f(A.bias[threadIdx.x]);
  __syncthreads();
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= A.pixels) return;
  const int w0 = (int)(pix % A.W);
  long long r = pix / A.W;
  const int h0 = (int)(r % A.H);
  r /= A.H;
  const int t0 = (int)(r % A.T);
  const int b = (int)(r / A.T);
  const int lH = A.H / A.pH, lW = A.W / A.pW;
  const unsigned short* xb = A.x + ((size_t)b * A.tile_rows + A.cls) * A.ldx;
  float acc0 = wsm[324], acc1 = wsm[325], acc2 = wsm[326];
  for (int dt = 0; dt < 3; ++dt) {
    const int t = t0 + dt - 1;
    if (t < 0 || t >= A.T) continue;
    const int tl = t / A.pT, tp = t - tl * A.pT;
    for (int dh = 0; dh < 3; ++dh) {
      const int hh = h0 + dh - 1;
      if (hh < 0 || hh >= A.H) continue;
      const int hl = hh / A.pH, hp = hh - hl * A.pH;
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        const int ww = w0 + dw - 1;
        if (ww < 0 || ww >= A.W) continue;
        const int wl = ww / A.pW, wp = ww - wl * A.pW;
        const size_t tokn = ((size_t)tl * lH + hl) * lW + wl;
        const int off = ((tp * A.pH + hp) * A.pW + wp) * 4;
        const u16x4 xv = *reinterpret_cast<const u16x4*>(xb + tokn * A.ldx + off);
        const float* wt = wsm + ((dt * 3 + dh) * 3 + dw) * 12;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const float xf = bf2f(xv[ci]);
          acc0 = fmaf(xf, wt[ci * 3 + 0], acc0);
          acc1 = fmaf(xf, wt[ci * 3 + 1], acc1);
          acc2 = fmaf(xf, wt[ci * 3 + 2], acc2);
        }
      }
    }
  }
  const size_t plane = (size_t)A.T * A.H * A.W;
  const size_t at = ((size_t)t0 * A.H + h0) * A.W + w0;
  unsigned short* yb = A.y + (size_t)b * 3 * plane + at;
  yb[0] = f2bf(acc0);
  yb[plane] = f2bf(acc1);
  yb[2 * plane] = f2bf(acc2);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct BlendArgs {
  const unsigned short* arena;     // raw tiles, tile k = [N, 3, P_k >= T_k, H_k, W_k] contiguous at element offset tab[k]
  const long long* tab;            // [nt nh nw] offsets; per axis (t, h, w): extents [n], output starts [n]; frame pitches [nt];
                                   // per axis: weights [n][e], w1 in the low and w2 in the high half of a word
  unsigned short* out;             // [N, 3, T, H, W] or NULL
  unsigned char* out_u8;           // [(N T), 3, H, W] or NULL; the HWC kernel: [N, T, H, W, 3]
  unsigned plane_units;            // H * (W / V)
  int T, H, W;
  int nt, nh, nw;
  int et, eh, ew;                  // blend extents in pixels
};

template <int V>
struct Pix {
  float v[V];
};

template <int V>
__device__ __forceinline__ Pix<V> load_pix(const unsigned short* p) {
  Pix<V> r;
  if constexpr (V == 8) {
    const u16x8 raw = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = bf2f(raw[i]);
  } else {
    r.v[0] = bf2f(*p);
  }
  return r;
}

// the tile that owns output coordinate o on one axis: the last one whose output start is not behind o
__device__ __forceinline__ int owner_of(const long long* start, int n, int o) {
  int k = n - 1;
  while (k > 0 && (int)start[k] > o) --k;
  return k;
}

// b = bf16(bf16(a w1) + bf16(b w2)): the reference's `a * (1 - p / e) + b * (p / e)` on bf16 tensors, the weights Python floats
// (double arithmetic) that torch applies at fp32 precision; `word` holds them as the host computed them
__device__ __forceinline__ float blend1(float a, float b, long long word) {
  const float w1 = __builtin_bit_cast(float, (unsigned)word), w2 = __builtin_bit_cast(float, (unsigned)((unsigned long long)word >> 32));
  return rbf(rbf(a * w1) + rbf(b * w2));
}

// HWC: one lane owns V pixels of a row and all three channels of them (blockIdx.z is the batch index, the lane loops over the channels)
// and writes uint8 [N, T, H, W, 3] through A.out_u8; else the channel is a grid axis (blockIdx.z = n * 3 + c) and the planar forms
// are written.  The element arithmetic is the same in both.
template <int V, bool HWC>
__global__ __launch_bounds__(256) void vit_tile_blend_kernel(BlendArgs A) {
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= A.plane_units) return;
  const unsigned Wv = (unsigned)A.W / V;
  const int y = (int)(u / Wv);
  const int x = (int)(u - (unsigned)y * Wv) * V;
  const int t = blockIdx.y;
  const int n = HWC ? (int)blockIdx.z : (int)(blockIdx.z / 3);

  const long long* ext_t = A.tab + (long long)A.nt * A.nh * A.nw;
  const long long* start_t = ext_t + A.nt;
  const long long* ext_h = start_t + A.nt;
  const long long* start_h = ext_h + A.nh;
  const long long* ext_w = start_h + A.nh;
  const long long* start_w = ext_w + A.nw;
  const long long* pitch_t = start_w + A.nw;
  const long long* wt_t = pitch_t + A.nt;
  const long long* wt_h = wt_t + (long long)A.nt * A.et;
  const long long* wt_w = wt_h + (long long)A.nh * A.eh;
  const int kt = owner_of(start_t, A.nt, t), kh = owner_of(start_h, A.nh, y), kw = owner_of(start_w, A.nw, x);
  const int Tk = (int)ext_t[kt], Hk = (int)ext_h[kh], Wk = (int)ext_w[kw];
  const int lt = t - (int)start_t[kt], ly = y - (int)start_h[kh], lx = x - (int)start_w[kw];
  const int tile = (kt * A.nh + kh) * A.nw + kw;
  const int Pk = (int)pitch_t[kt];

  // the V pixels of plane nc = n * 3 + c: the owner's values behind the RAW-neighbour blends in t, h, w order
  auto blended = [&](size_t nc) {
    auto at = [&](int k, int Te, int He, int We, int tt, int yy, int xx) {   // Te: the frames the tile's storage holds per channel
      return A.arena + A.tab[k] + (((nc * Te + tt) * He + yy) * (size_t)We + xx);
    };
    Pix<V> b = load_pix<V>(at(tile, Pk, Hk, Wk, lt, ly, lx));
    if (kt > 0) {
      const int Ta = (int)ext_t[kt - 1];
      const int e = min(min(Ta, Tk), A.et);
      if (lt < e) {
        const Pix<V> a = load_pix<V>(at(tile - A.nh * A.nw, (int)pitch_t[kt - 1], Hk, Wk, Ta - e + lt, ly, lx));
        const long long w = wt_t[(long long)kt * A.et + lt];
#pragma unroll
        for (int i = 0; i < V; ++i) b.v[i] = blend1(a.v[i], b.v[i], w);
      }
    }
    if (kh > 0) {
      const int Ha = (int)ext_h[kh - 1];
      const int e = min(min(Ha, Hk), A.eh);
      if (ly < e) {
        const Pix<V> a = load_pix<V>(at(tile - A.nw, Pk, Ha, Wk, lt, Ha - e + ly, lx));
        const long long w = wt_h[(long long)kh * A.eh + ly];
#pragma unroll
        for (int i = 0; i < V; ++i) b.v[i] = blend1(a.v[i], b.v[i], w);
      }
    }
    if (kw > 0) {
      const int Wa = (int)ext_w[kw - 1];
      const int e = min(min(Wa, Wk), A.ew);
      if (lx < e) {                                            // V == 8: e and lx are multiples of 8, all 8 pixels are inside
        const Pix<V> a = load_pix<V>(at(tile - 1, Pk, Hk, Wa, lt, ly, Wa - e + lx));
        const long long* w = wt_w + (long long)kw * A.ew + lx;
#pragma unroll
        for (int i = 0; i < V; ++i) b.v[i] = blend1(a.v[i], b.v[i], w[i]);
      }
    }
    return b;
  };
  // `VaeHelper.decode`: bf16(bf16(x 127.5) + 127.5), clamp(0, 255), truncation
  auto quantise = [](float v) {
    const float f = rbf(rbf(v * 127.5f) + 127.5f);
    return (unsigned)(int)fminf(fmaxf(f, 0.f), 255.f);
  };

  if constexpr (HWC) {
    unsigned q[3][V];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const Pix<V> b = blended((size_t)n * 3 + c);
#pragma unroll
      for (int i = 0; i < V; ++i) q[c][i] = quantise(b.v[i]);
    }
    unsigned char* op = A.out_u8 + ((((size_t)n * A.T + t) * A.H + y) * (size_t)A.W + x) * 3;
    if constexpr (V == 8) {                                    // 24 contiguous bytes: byte 3 i + c is channel c of pixel i
      unsigned w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 24; ++k) w[k / 4] |= q[k % 3][k / 3] << (8 * (k % 4));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        u32x2 o;
        o[0] = w[2 * k];
        o[1] = w[2 * k + 1];
        reinterpret_cast<u32x2*>(op)[k] = o;
      }
    } else {
      op[0] = (unsigned char)q[0][0];
      op[1] = (unsigned char)q[1][0];
      op[2] = (unsigned char)q[2][0];
    }
  } else {
    const int c = blockIdx.z % 3;
    const size_t nc = (size_t)n * 3 + c;
    const Pix<V> b = blended(nc);
    if (A.out) {
      unsigned short* op = A.out + (((nc * A.T + t) * A.H + y) * (size_t)A.W + x);
      if constexpr (V == 8) {
        u16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = f2bf(b.v[i]);
        *reinterpret_cast<u16x8*>(op) = o;
      } else {
        *op = f2bf(b.v[0]);
      }
    }
    if (A.out_u8) {
      unsigned q[V];
#pragma unroll
      for (int i = 0; i < V; ++i) q[i] = quantise(b.v[i]);
      unsigned char* op = A.out_u8 + (((((size_t)n * A.T + t) * 3 + c) * A.H + y) * (size_t)A.W + x);
      if constexpr (V == 8) {
        u32x2 o;
        o[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        o[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
        *reinterpret_cast<u32x2*>(op) = o;
      } else {
        *op = (unsigned char)q[0];
      }
    }
  }
}

}  // namespace vit
}  // namespace ifx

using namespace ifx;

extern "C" int ifx_vit_head_prep(ifx_bf16* qkv, int32_t ld, const ifx_bf16* sin_table, const ifx_bf16* cos_table, int32_t batch,
                                 int32_t tokens, int32_t heads, int32_t cls_tokens, int32_t do_norm, int32_t do_rope, float eps,
                                 void* stream) {
  IFX_REQUIRE(qkv, "ifx_vit_head_prep: null qkv");
  IFX_REQUIRE(batch >= 1 && heads >= 1, "ifx_vit_head_prep: empty batch (%d) / heads (%d)", batch, heads);
  IFX_REQUIRE(tokens >= 1, "ifx_vit_head_prep: tokens (%d) must be >= 1", tokens);
  IFX_REQUIRE(ld % 8 == 0, "ifx_vit_head_prep: ld (%d) must be a multiple of 8", ld);
  IFX_REQUIRE((long long)3 * heads * vit::HD <= ld, "ifx_vit_head_prep: 3 x %d heads x 64 channels do not fit ld (%d)", heads, ld);
  IFX_REQUIRE(cls_tokens >= 0 && cls_tokens <= tokens, "ifx_vit_head_prep: cls_tokens (%d) outside [0, tokens %d]", cls_tokens, tokens);
  if (do_rope) IFX_REQUIRE(sin_table && cos_table, "ifx_vit_head_prep: the rotation needs the sin and cos tables");
  IFX_REQUIRE(((uintptr_t)qkv | (uintptr_t)sin_table | (uintptr_t)cos_table) % 16 == 0,
              "ifx_vit_head_prep: qkv and the tables must be 16-byte aligned");
  if (!do_norm && !do_rope) return IFX_OK;
  vit::PrepArgs a;
  a.qkv = qkv;
  a.sin_t = sin_table;
  a.cos_t = cos_table;
  a.units = (long long)batch * tokens * 3 * heads;
  a.ld = ld;
  a.tokens = tokens;
  a.heads = heads;
  a.cls = cls_tokens;
  a.do_norm = do_norm != 0;
  a.do_rope = do_rope != 0;
  a.eps = eps;
  const long long blocks = (a.units + 31) / 32;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_vit_head_prep: launch too large");
  hipLaunchKernelGGL(vit::vit_head_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_vit_head_prep");
}

extern "C" int ifx_vit_attention(const ifx_bf16* q, int32_t ldq, const ifx_bf16* k, int32_t ldk, const ifx_bf16* v, int32_t ldv,
                                 ifx_bf16* out, int32_t ldo, int32_t batch, int32_t tokens, int32_t heads, void* stream) {
  IFX_REQUIRE(q && k && v && out, "ifx_vit_attention: null argument");
  IFX_REQUIRE(batch >= 1 && heads >= 1, "ifx_vit_attention: empty batch (%d) / heads (%d)", batch, heads);
  IFX_REQUIRE(tokens >= 1, "ifx_vit_attention: tokens (%d) must be >= 1", tokens);
  IFX_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0,
              "ifx_vit_attention: row strides (%d, %d, %d, %d) must be multiples of 8", ldq, ldk, ldv, ldo);
  const long long width = (long long)heads * vit::HD;
  IFX_REQUIRE(width <= ldq && width <= ldk && width <= ldv && width <= ldo,
              "ifx_vit_attention: %d heads x 64 channels do not fit the row strides (%d, %d, %d, %d)", heads, ldq, ldk, ldv, ldo);
  IFX_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)out % 8 == 0,
              "ifx_vit_attention: q / k / v must be 16-byte aligned, out 8-byte aligned");
  vit::AttnArgs a;
  a.q = q;
  a.k = k;
  a.v = v;
  a.out = out;
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.ldo = ldo;
  a.tokens = tokens;
  a.heads = heads;
  a.q_tiles = (tokens + 127) / 128;
  const long long blocks = (long long)batch * heads * a.q_tiles;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_vit_attention: launch too large");
  hipLaunchKernelGGL(vit::vit_attention_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_vit_attention");
}

extern "C" int ifx_vit_unpatch_conv(const ifx_bf16* x, int32_t ldx, int32_t tile_rows, int32_t cls_tokens, const ifx_bf16* weight,
                                    const ifx_bf16* bias, ifx_bf16* y, int32_t batch, int32_t t_out, int32_t h_out, int32_t w_out,
                                    int32_t patch_t, int32_t patch_h, int32_t patch_w, int32_t channels, void* stream) {
  IFX_REQUIRE(x && weight && bias && y, "ifx_vit_unpatch_conv: null argument");
  IFX_REQUIRE(channels == 4, "ifx_vit_unpatch_conv: channels %d not built (4 only)", channels);
  IFX_REQUIRE(batch >= 1 && t_out >= 1 && h_out >= 1 && w_out >= 1, "ifx_vit_unpatch_conv: empty output (%d x %d x %d x %d)", batch, t_out,
              h_out, w_out);
  IFX_REQUIRE(patch_t >= 1 && patch_h >= 1 && patch_w >= 1 && t_out % patch_t == 0 && h_out % patch_h == 0 && w_out % patch_w == 0,
              "ifx_vit_unpatch_conv: patch %d x %d x %d does not divide the output %d x %d x %d", patch_t, patch_h, patch_w, t_out, h_out,
              w_out);
  IFX_REQUIRE(ldx % 8 == 0, "ifx_vit_unpatch_conv: ldx (%d) must be a multiple of 8", ldx);
  const long long width = (long long)patch_t * patch_h * patch_w * channels;
  IFX_REQUIRE(width <= ldx, "ifx_vit_unpatch_conv: a patch row of %lld channels does not fit ldx (%d)", width, ldx);
  const long long tokens = (long long)(t_out / patch_t) * (h_out / patch_h) * (w_out / patch_w);
  IFX_REQUIRE(cls_tokens >= 0 && tokens + cls_tokens <= 0x7fffffffLL && tile_rows == tokens + cls_tokens,
              "ifx_vit_unpatch_conv: tile_rows (%d) is not cls_tokens (%d) + %lld patch tokens", tile_rows, cls_tokens, tokens);
  IFX_REQUIRE((uintptr_t)x % 8 == 0, "ifx_vit_unpatch_conv: x must be 8-byte aligned");
  vit::ConvArgs a;
  a.x = x;
  a.w = weight;
  a.bias = bias;
  a.y = y;
  a.pixels = (long long)batch * t_out * h_out * w_out;
  a.ldx = ldx;
  a.tile_rows = tile_rows;
  a.cls = cls_tokens;
  a.T = t_out;
  a.H = h_out;
  a.W = w_out;
  a.pT = patch_t;
  a.pH = patch_h;
  a.pW = patch_w;
  const long long blocks = (a.pixels + 255) / 256;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_vit_unpatch_conv: launch too large");
  hipLaunchKernelGGL(vit::vit_unpatch_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_vit_unpatch_conv");
}

extern "C" int ifx_vit_tile_blend(const ifx_bf16* arena, const int64_t* table, ifx_bf16* out, uint8_t* out_u8, int32_t batch,
                                  int32_t t_out, int32_t h_out, int32_t w_out, int32_t tiles_t, int32_t tiles_h, int32_t tiles_w,
                                  int32_t blend_t, int32_t blend_h, int32_t blend_w, int32_t limit_t, int32_t limit_h, int32_t limit_w,
                                  int32_t vec_x, void* stream) {
  IFX_REQUIRE(arena && table, "ifx_vit_tile_blend: null arena / table");
  IFX_REQUIRE(out || out_u8, "ifx_vit_tile_blend: both outputs are null (out or out_u8 is required)");
  IFX_REQUIRE(batch >= 1 && t_out >= 1 && h_out >= 1 && w_out >= 1, "ifx_vit_tile_blend: empty output (%d x %d x %d x %d)", batch, t_out,
              h_out, w_out);
  IFX_REQUIRE(tiles_t >= 1 && tiles_h >= 1 && tiles_w >= 1, "ifx_vit_tile_blend: empty tile grid (%d x %d x %d)", tiles_t, tiles_h, tiles_w);
  IFX_REQUIRE((long long)tiles_t * tiles_h * tiles_w <= 0x7fffffffLL, "ifx_vit_tile_blend: tile grid too large");
  IFX_REQUIRE(limit_t >= 1 && limit_h >= 1 && limit_w >= 1, "ifx_vit_tile_blend: limits (%d, %d, %d) must be >= 1", limit_t, limit_h,
              limit_w);
  IFX_REQUIRE(blend_t >= 0 && blend_h >= 0 && blend_w >= 0, "ifx_vit_tile_blend: blend extents (%d, %d, %d) must be >= 0", blend_t,
              blend_h, blend_w);
  IFX_REQUIRE(blend_t <= limit_t && blend_h <= limit_h && blend_w <= limit_w,
              "ifx_vit_tile_blend: a blend extent (%d, %d, %d) is larger than its limit (%d, %d, %d)", blend_t, blend_h, blend_w, limit_t,
              limit_h, limit_w);
  // every tile keeps between one position and `limit` positions of an axis
  IFX_REQUIRE(t_out >= tiles_t && t_out <= (long long)tiles_t * limit_t, "ifx_vit_tile_blend: t_out (%d) is not what %d tiles of limit %d give",
              t_out, tiles_t, limit_t);
  IFX_REQUIRE(h_out >= tiles_h && h_out <= (long long)tiles_h * limit_h, "ifx_vit_tile_blend: h_out (%d) is not what %d tiles of limit %d give",
              h_out, tiles_h, limit_h);
  IFX_REQUIRE(w_out >= tiles_w && w_out <= (long long)tiles_w * limit_w, "ifx_vit_tile_blend: w_out (%d) is not what %d tiles of limit %d give",
              w_out, tiles_w, limit_w);
  IFX_REQUIRE((uintptr_t)table % 8 == 0, "ifx_vit_tile_blend: table must be 8-byte aligned");
  if (vec_x) {
    IFX_REQUIRE(w_out % 8 == 0 && blend_w % 8 == 0 && (tiles_w == 1 || limit_w % 8 == 0),
                "ifx_vit_tile_blend: vec_x needs w_out (%d), blend_w (%d) and limit_w (%d) to be multiples of 8", w_out, blend_w, limit_w);
    IFX_REQUIRE(((uintptr_t)arena | (uintptr_t)out) % 16 == 0 && (uintptr_t)out_u8 % 8 == 0,
                "ifx_vit_tile_blend: vec_x needs arena and out 16-byte aligned, out_u8 8-byte aligned");
  } else {
    IFX_REQUIRE(((uintptr_t)arena | (uintptr_t)out) % 2 == 0, "ifx_vit_tile_blend: arena and out must be 2-byte aligned");
  }
  vit::BlendArgs a;
  a.arena = arena;
  a.tab = (const long long*)table;
  a.out = out;
  a.out_u8 = out_u8;
  const long long plane_units = (long long)h_out * (vec_x ? w_out / 8 : w_out);
  IFX_REQUIRE(plane_units <= 0x7fffffffLL && t_out <= 65535 && (long long)batch * 3 <= 65535,
              "ifx_vit_tile_blend: launch too large (%d x 3 planes of %d frames of %lld units)", batch, t_out, plane_units);
  a.plane_units = (unsigned)plane_units;
  a.T = t_out;
  a.H = h_out;
  a.W = w_out;
  a.nt = tiles_t;
  a.nh = tiles_h;
  a.nw = tiles_w;
  a.et = blend_t;
  a.eh = blend_h;
  a.ew = blend_w;
  const dim3 grid((unsigned)((plane_units + 255) / 256), (unsigned)t_out, (unsigned)batch * 3);
  if (vec_x)
    hipLaunchKernelGGL((vit::vit_tile_blend_kernel<8, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((vit::vit_tile_blend_kernel<1, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_vit_tile_blend");
}

extern "C" int ifx_vit_tile_blend_hwc(const ifx_bf16* arena, const int64_t* table, uint8_t* out_hwc, int32_t batch, int32_t t_out,
                                      int32_t h_out, int32_t w_out, int32_t tiles_t, int32_t tiles_h, int32_t tiles_w, int32_t blend_t,
                                      int32_t blend_h, int32_t blend_w, int32_t limit_t, int32_t limit_h, int32_t limit_w, int32_t vec_x,
                                      void* stream) {
  IFX_REQUIRE(arena && table, "ifx_vit_tile_blend_hwc: null arena / table");
  IFX_REQUIRE(out_hwc, "ifx_vit_tile_blend_hwc: null out_hwc");
  IFX_REQUIRE(batch >= 1 && t_out >= 1 && h_out >= 1 && w_out >= 1, "ifx_vit_tile_blend_hwc: empty output (%d x %d x %d x %d)", batch,
              t_out, h_out, w_out);
  IFX_REQUIRE(tiles_t >= 1 && tiles_h >= 1 && tiles_w >= 1, "ifx_vit_tile_blend_hwc: empty tile grid (%d x %d x %d)", tiles_t, tiles_h,
              tiles_w);
  IFX_REQUIRE((long long)tiles_t * tiles_h * tiles_w <= 0x7fffffffLL, "ifx_vit_tile_blend_hwc: tile grid too large");
  IFX_REQUIRE(limit_t >= 1 && limit_h >= 1 && limit_w >= 1, "ifx_vit_tile_blend_hwc: limits (%d, %d, %d) must be >= 1", limit_t, limit_h,
              limit_w);
  IFX_REQUIRE(blend_t >= 0 && blend_h >= 0 && blend_w >= 0, "ifx_vit_tile_blend_hwc: blend extents (%d, %d, %d) must be >= 0", blend_t,
              blend_h, blend_w);
  IFX_REQUIRE(blend_t <= limit_t && blend_h <= limit_h && blend_w <= limit_w,
              "ifx_vit_tile_blend_hwc: a blend extent (%d, %d, %d) is larger than its limit (%d, %d, %d)", blend_t, blend_h, blend_w,
              limit_t, limit_h, limit_w);
  IFX_REQUIRE(t_out >= tiles_t && t_out <= (long long)tiles_t * limit_t,
              "ifx_vit_tile_blend_hwc: t_out (%d) is not what %d tiles of limit %d give", t_out, tiles_t, limit_t);
  IFX_REQUIRE(h_out >= tiles_h && h_out <= (long long)tiles_h * limit_h,
              "ifx_vit_tile_blend_hwc: h_out (%d) is not what %d tiles of limit %d give", h_out, tiles_h, limit_h);
  IFX_REQUIRE(w_out >= tiles_w && w_out <= (long long)tiles_w * limit_w,
              "ifx_vit_tile_blend_hwc: w_out (%d) is not what %d tiles of limit %d give", w_out, tiles_w, limit_w);
  IFX_REQUIRE((uintptr_t)table % 8 == 0, "ifx_vit_tile_blend_hwc: table must be 8-byte aligned");
  if (vec_x) {
    IFX_REQUIRE(w_out % 8 == 0 && blend_w % 8 == 0 && (tiles_w == 1 || limit_w % 8 == 0),
                "ifx_vit_tile_blend_hwc: vec_x needs w_out (%d), blend_w (%d) and limit_w (%d) to be multiples of 8", w_out, blend_w,
                limit_w);
    IFX_REQUIRE((uintptr_t)arena % 16 == 0 && (uintptr_t)out_hwc % 8 == 0,
                "ifx_vit_tile_blend_hwc: vec_x needs arena 16-byte aligned, out_hwc 8-byte aligned");
  } else {
    IFX_REQUIRE((uintptr_t)arena % 2 == 0, "ifx_vit_tile_blend_hwc: arena must be 2-byte aligned");
  }
  vit::BlendArgs a;
  a.arena = arena;
  a.tab = (const long long*)table;
  a.out = nullptr;
  a.out_u8 = out_hwc;
  const long long plane_units = (long long)h_out * (vec_x ? w_out / 8 : w_out);
  IFX_REQUIRE(plane_units <= 0x7fffffffLL && t_out <= 65535 && batch <= 65535,
              "ifx_vit_tile_blend_hwc: launch too large (%d samples of %d frames of %lld units)", batch, t_out, plane_units);
  a.plane_units = (unsigned)plane_units;
  a.T = t_out;
  a.H = h_out;
  a.W = w_out;
  a.nt = tiles_t;
  a.nh = tiles_h;
  a.nw = tiles_w;
  a.et = blend_t;
  a.eh = blend_h;
  a.ew = blend_w;
  const dim3 grid((unsigned)((plane_units + 255) / 256), (unsigned)t_out, (unsigned)batch);
  if (vec_x)
    hipLaunchKernelGGL((vit::vit_tile_blend_kernel<8, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((vit::vit_tile_blend_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_vit_tile_blend_hwc");
}

// MAGI ViT-VAE encoder kernels (prefix-video encode of the i2v / v2v modes), gfx950 only: what `ViTEncoder`
// (inferix/models/magi/vae/vae_module.py:409-558) and `TileProcessor.tiled_encode` (inferix/distributed/parallelism/tile_parallel.py:
// 254-346) need besides ifx_layernorm, ifx_gemm_bf16 and the block kernels of ifx_vit.hip.
//
//   vit_patch_rows_kernel    `PatchEmbed.proj` is Conv3d(3 -> D, kernel = stride = patch), i.e. a GEMM whose A operand is the video cut
//                            into patches: this kernel gathers the pixels of every patch into one token row, K order (c, t, h, w) as in
//                            `weight.flatten(1)`.  The video is a base pointer with five element strides (a window of a larger video
//                            and the stride-0 expand of a single frame cost no copy); the tiles of one launch are origins in the kernel
//                            arguments, validated on the host.  With 8-pixel-wide patches a lane moves the 8 pixels of one patch row
//                            (16 bytes written, 16 or 8 read) and consecutive lanes write consecutive chunks of a token row; any other
//                            geometry goes one element per lane.  uint8 pixels become bf16(fp32(v) / 127.5f - 1.0f), the
//                            normalisation of `VaeHelper.encode`.
//   vit_latent_head_kernel   `ViTEncoder.forward` :542-557: the final affine LayerNorm (result a bf16 tensor), `last_layer`
//                            (bf16(fp32 dot + bias) per output channel), optionally `norm_code` (fp32 quotient by the L2 norm over the
//                            channels, one rounding), class rows dropped, stored channel-first.  One wave per token row; the C2 x D
//                            weight sits in LDS (64 KiB at 32 x 1024), loaded once per workgroup, which then walks rows.
//   vit_latent_blend_kernel  the blend chain of `tiled_encode` on the encoded tiles, IN PLACE as the reference does it (no clone: a
//                            tile is blended against its already blended neighbours).  One launch per anti-diagonal f + i + j of the
//                            tile grid: a tile's three neighbours lie on the diagonal before it, so a launch reads finished tiles only
//                            and every thread writes nothing but its own element, which it takes through the temporal, the vertical
//                            and the horizontal blend in that order.  No device-side wait, no atomic.
#include <algorithm>

#include "ifx_launch.h"
#include "ifx_rows.h"

namespace ifx {
namespace vitenc {

constexpr int MAX_TILES = 64;      // tile origins one launch carries in its arguments

struct PatchArgs {
  const void* video;
  unsigned short* rows;
  long long sn, sc, st, sh, sw;    // element strides of the video
  long long units;                 // per (tile, sample): tokens * chunks (vector path) or tokens * K (element path)
  int ld, batch, rows_per_tile, cls;
  int pT, pH, pW, lH, lW;
  int tile0;                       // first tile of this launch (row offset tile0 * batch * rows_per_tile)
  int t0[MAX_TILES], h0[MAX_TILES], w0[MAX_TILES];
};

__device__ __forceinline__ unsigned short pixel_u8(unsigned char v) { return f2bf((float)v / 127.5f - 1.0f); }

template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void vit_patch_rows_kernel(PatchArgs A) {
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= A.units) return;
  const int tile = blockIdx.y / A.batch, n = blockIdx.y - tile * A.batch;
  const int per_tok = VEC ? 3 * A.pT * A.pH : 3 * A.pT * A.pH * A.pW;      // chunks or elements of one token row
  const int tok = (int)(u / per_tok);
  int k = (int)(u - (long long)tok * per_tok);
  const int col = VEC ? k * 8 : k;
  int pw = 0;
  if (!VEC) {
    pw = k % A.pW;
    k /= A.pW;
  }
  const int ph = k % A.pH;
  k /= A.pH;
  const int pt = k % A.pT, c = k / A.pT;
  const int lw = tok % A.lW;
  const int r = tok / A.lW;
  const int lh = r % A.lH, lt = r / A.lH;
  const long long src = n * A.sn + c * A.sc + (long long)(A.t0[tile] + lt * A.pT + pt) * A.st +
                        (long long)(A.h0[tile] + lh * A.pH + ph) * A.sh + (long long)(A.w0[tile] + lw * A.pW + pw) * A.sw;
  const long long row = ((long long)(A.tile0 + tile) * A.batch + n) * A.rows_per_tile + A.cls + tok;
  unsigned short* dst = A.rows + row * A.ld + col;
  if constexpr (VEC) {
    u16x8 o;
    if constexpr (U8) {
      const u32x2 raw = *reinterpret_cast<const u32x2*>(static_cast<const unsigned char*>(A.video) + src);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = pixel_u8((unsigned char)(raw[i >> 2] >> (8 * (i & 3))));
    } else {
      o = *reinterpret_cast<const u16x8*>(static_cast<const unsigned short*>(A.video) + src);
    }
    *reinterpret_cast<u16x8*>(dst) = o;
  } else {
    if constexpr (U8) *dst = pixel_u8(static_cast<const unsigned char*>(A.video)[src]);
    else *dst = static_cast<const unsigned short*>(A.video)[src];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct HeadArgs {
  const unsigned short* x;         // [batch * rows_per_tile, D], row stride ld
  const unsigned short* gamma;
  const unsigned short* beta;
  const unsigned short* w;         // [C2, D]
  const unsigned short* bias;      // [C2]
  unsigned short* out;             // sample b at out + b * out_stride: [store, tokens]
  long long out_stride;
  long long rows;                  // batch * rows_per_tile
  int ld, D, C2, store, rows_per_tile, cls, norm_code;
  float eps;
};

template <int NCH, int CMAX>
__global__ __launch_bounds__(256) void vit_latent_head_kernel(HeadArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_smem[];
  unsigned short* wsm = reinterpret_cast<unsigned short*>(head_smem);          // [C2][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = A.C2 * A.D / 8;
  for (int i = threadIdx.x; i < chunks; i += 256)
    *reinterpret_cast<u16x8*>(wsm + i * 8) = *reinterpret_cast<const u16x8*>(A.w + (size_t)i * 8);
  u16x8 g[NCH], b[NCH];
  load_chunks<NCH>(g, A.gamma, A.D, lane);
  load_chunks<NCH>(b, A.beta, A.D, lane);
  const float my_bias = lane < A.C2 ? bf2f(A.bias[lane]) : 0.f;
  __syncthreads();
  const int tokens = A.rows_per_tile - A.cls;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < A.rows; row += (long long)gridDim.x * 4) {
    const long long bi = row / A.rows_per_tile;
    const int tok = (int)(row - bi * A.rows_per_tile) - A.cls;
    if (tok < 0) continue;                                        // class rows: wave-uniform
    u16x8 raw[NCH];
    load_chunks<NCH>(raw, A.x + row * A.ld, A.D, lane);
    Row<NCH> r;
    r.from(raw, A.D, lane);
    float mean, rstd;
    ln_stats(r, A.D, A.eps, lane, mean, rstd);
    float y[NCH][8];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const bool ok = c * 512 + lane * 8 < A.D;
#pragma unroll
      for (int i = 0; i < 8; ++i) y[c][i] = ok ? rbf((r.v[c][i] - mean) * rstd * bf2f(g[c][i]) + bf2f(b[c][i])) : 0.f;
    }
    float mine = 0.f, ssq = 0.f;                                  // lane c keeps channel c
#pragma unroll
    for (int ch = 0; ch < CMAX; ++ch) {
      if (ch < A.C2) {
        float p = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int col = c * 512 + lane * 8;
          const u16x8 wv = *reinterpret_cast<const u16x8*>(wsm + ch * A.D + (col < A.D ? col : 0));
#pragma unroll
          for (int i = 0; i < 8; ++i) p = fmaf(y[c][i], bf2f(wv[i]), p);      // y is zero beyond D
        }
        const float dot = wave_sum(p);
        const float bch = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_bias), ch));
        const float v = rbf(dot + bch);
        ssq += v * v;
        if (lane == ch) mine = v;
      }
    }
    if (A.norm_code) mine = mine / sqrtf(ssq);
    if (lane < A.store) A.out[bi * A.out_stride + (long long)lane * tokens + tok] = f2bf(mine);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct LatentBlendArgs {
  unsigned short* arena;           // tile k = [NC, T_k, H_k, W_k] contiguous at element offset tab[k]
  const long long* tab;            // [tiles] offsets; per axis (t, h, w): extents [n]; per axis: weights [n][e]; [tiles] tile ids by diagonal
  long long arena_elements;
  int nc;                          // samples x channels
  int nt, nh, nw;
  int et, eh, ew;                  // blend extents in latents
  int first;                       // position in the diagonal-ordered id list of this launch's first tile
};

__device__ __forceinline__ float blend1(float a, float b, long long word) {
  const float w1 = __builtin_bit_cast(float, (unsigned)word), w2 = __builtin_bit_cast(float, (unsigned)((unsigned long long)word >> 32));
  return rbf(rbf(a * w1) + rbf(b * w2));
}

__global__ __launch_bounds__(256) void vit_latent_blend_kernel(LatentBlendArgs A) {
  const int tiles = A.nt * A.nh * A.nw;
  const long long* ext_t = A.tab + tiles;
  const long long* ext_h = ext_t + A.nt;
  const long long* ext_w = ext_h + A.nh;
  const long long* wt_t = ext_w + A.nw;
  const long long* wt_h = wt_t + (long long)A.nt * A.et;
  const long long* wt_w = wt_h + (long long)A.nh * A.eh;
  const long long* ids = wt_w + (long long)A.nw * A.ew;
  const int tile = (int)ids[A.first + blockIdx.y];
  if (tile < 0 || tile >= tiles) return;
  const int j = tile % A.nw, i = (tile / A.nw) % A.nh, f = tile / (A.nw * A.nh);
  const int Tk = (int)ext_t[f], Hk = (int)ext_h[i], Wk = (int)ext_w[j];
  const long long per = (long long)Tk * Hk * Wk;
  const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
  if (u >= per * A.nc) return;
  const int c = (int)(u / per);
  long long r = u - c * per;
  const int x = (int)(r % Wk);
  r /= Wk;
  const int y = (int)(r % Hk), t = (int)(r / Hk);
  const long long own = A.tab[tile] + u;
  if (own < 0 || own >= A.arena_elements) return;
  // every address is checked against the arena: the table's contents come from the caller
  auto load = [&](int k, int Te, int He, int We, int tt, int yy, int xx, float& v) {
    const long long at = A.tab[k] + ((((long long)c * Te + tt) * He + yy) * We + xx);
    const bool ok = at >= 0 && at < A.arena_elements;
    if (ok) v = bf2f(A.arena[at]);
    return ok;
  };
  float b = bf2f(A.arena[own]), a = 0.f;
  bool changed = false;
  if (f > 0) {
    const int Ta = (int)ext_t[f - 1];
    const int e = min(min(Ta, Tk), A.et);
    if (t < e && load(tile - A.nh * A.nw, Ta, Hk, Wk, Ta - e + t, y, x, a)) {
      b = blend1(a, b, wt_t[(long long)f * A.et + t]);
      changed = true;
    }
  }
  if (i > 0) {
    const int Ha = (int)ext_h[i - 1];
    const int e = min(min(Ha, Hk), A.eh);
    if (y < e && load(tile - A.nw, Tk, Ha, Wk, t, Ha - e + y, x, a)) {
      b = blend1(a, b, wt_h[(long long)i * A.eh + y]);
      changed = true;
    }
  }
  if (j > 0) {
    const int Wa = (int)ext_w[j - 1];
    const int e = min(min(Wa, Wk), A.ew);
    if (x < e && load(tile - 1, Tk, Hk, Wa, t, y, Wa - e + x, a)) {
      b = blend1(a, b, wt_w[(long long)j * A.ew + x]);
      changed = true;
    }
  }
  if (changed) A.arena[own] = f2bf(b);
}

}  // namespace vitenc
}  // namespace ifx

using namespace ifx;

extern "C" int ifx_vit_patch_rows(const void* video, int32_t is_uint8, const int64_t* strides, const int64_t* dims, const int64_t* tiles,
                                  int32_t n_tiles, ifx_bf16* rows, int32_t ld, int32_t cls_tokens, int32_t patch_t, int32_t patch_h,
                                  int32_t patch_w, int32_t lat_t, int32_t lat_h, int32_t lat_w, void* stream) {
  IFX_REQUIRE(video && strides && dims && tiles && rows, "ifx_vit_patch_rows: null argument");
  IFX_REQUIRE(patch_t >= 1 && patch_h >= 1 && patch_w >= 1 && (long long)3 * patch_t * patch_h * patch_w <= 0x7fffffffLL,
              "ifx_vit_patch_rows: bad patch %d x %d x %d", patch_t, patch_h, patch_w);
  const long long K = (long long)3 * patch_t * patch_h * patch_w;
  IFX_REQUIRE(n_tiles >= 1 && cls_tokens >= 0, "ifx_vit_patch_rows: n_tiles (%d) must be >= 1, cls_tokens (%d) >= 0", n_tiles, cls_tokens);
  IFX_REQUIRE(lat_t >= 1 && lat_h >= 1 && lat_w >= 1, "ifx_vit_patch_rows: latent shape %d x %d x %d: an extent is smaller than one patch",
              lat_t, lat_h, lat_w);
  const long long N = dims[0], Cc = dims[1], T = dims[2], H = dims[3], W = dims[4];
  IFX_REQUIRE(N >= 1 && N <= 65535 && Cc == 3 && T >= 1 && H >= 1 && W >= 1 && T <= 0x7fffffffLL && H <= 0x7fffffffLL && W <= 0x7fffffffLL,
              "ifx_vit_patch_rows: video dims [%lld, %lld, %lld, %lld, %lld] (3 channels, 1 .. 65535 samples)", N, Cc, T, H, W);
  for (int a = 0; a < 5; ++a) IFX_REQUIRE(strides[a] >= 0, "ifx_vit_patch_rows: stride %d is negative (%lld)", a, (long long)strides[a]);
  const long long tokens = (long long)lat_t * lat_h * lat_w;
  IFX_REQUIRE(tokens + cls_tokens <= 0x7fffffffLL, "ifx_vit_patch_rows: %lld tokens per tile", tokens);
  IFX_REQUIRE(ld >= K, "ifx_vit_patch_rows: a patch row of %lld elements does not fit ld (%d)", K, ld);
  IFX_REQUIRE((uintptr_t)rows % 2 == 0 && (is_uint8 || (uintptr_t)video % 2 == 0), "ifx_vit_patch_rows: video / rows must be 2-byte aligned");
  bool vec = patch_w == 8 && strides[4] == 1 && ld % 8 == 0 && (uintptr_t)rows % 16 == 0;
  const int src_align = is_uint8 ? 8 : 16, esz = is_uint8 ? 1 : 2;
  vec = vec && (uintptr_t)video % src_align == 0;
  for (int a = 0; a < 4; ++a) vec = vec && (strides[a] * esz) % src_align == 0;
  for (int k = 0; k < n_tiles; ++k) {
    const int64_t* t = tiles + (size_t)k * 6;
    const long long o[3] = {t[0], t[1], t[2]}, e[3] = {t[3], t[4], t[5]}, full[3] = {T, H, W};
    const int p[3] = {patch_t, patch_h, patch_w}, lat[3] = {lat_t, lat_h, lat_w};
    for (int a = 0; a < 3; ++a) {
      IFX_REQUIRE(o[a] >= 0 && e[a] >= 0 && o[a] + e[a] <= full[a], "ifx_vit_patch_rows: tile %d axis %d: [%lld, %lld) outside the video (%lld)",
                  k, a, o[a], o[a] + e[a], full[a]);
      IFX_REQUIRE(e[a] >= p[a], "ifx_vit_patch_rows: tile %d axis %d: extent %lld is smaller than one patch (%d)", k, a, e[a], p[a]);
      IFX_REQUIRE(e[a] / p[a] == lat[a], "ifx_vit_patch_rows: tile %d axis %d: extent %lld / patch %d is not the launch's latent extent %d", k,
                  a, e[a], p[a], lat[a]);
    }
    vec = vec && t[2] % 8 == 0;
  }
  vitenc::PatchArgs a;
  a.video = video;
  a.rows = rows;
  a.sn = strides[0];
  a.sc = strides[1];
  a.st = strides[2];
  a.sh = strides[3];
  a.sw = strides[4];
  a.units = tokens * (vec ? K / 8 : K);
  a.ld = ld;
  a.batch = (int)N;
  a.rows_per_tile = (int)(tokens + cls_tokens);
  a.cls = cls_tokens;
  a.pT = patch_t;
  a.pH = patch_h;
  a.pW = patch_w;
  a.lH = lat_h;
  a.lW = lat_w;
  const long long blocks = (a.units + 255) / 256;
  IFX_REQUIRE(blocks <= 0x7fffffffLL, "ifx_vit_patch_rows: launch too large");
  const int per_launch = (int)std::min<long long>(vitenc::MAX_TILES, 65535 / N);
  for (int k0 = 0; k0 < n_tiles; k0 += per_launch) {
    const int n = std::min(per_launch, n_tiles - k0);
    a.tile0 = k0;
    for (int k = 0; k < n; ++k) {
      a.t0[k] = (int)tiles[(size_t)(k0 + k) * 6 + 0];
      a.h0[k] = (int)tiles[(size_t)(k0 + k) * 6 + 1];
      a.w0[k] = (int)tiles[(size_t)(k0 + k) * 6 + 2];
    }
    const dim3 grid((unsigned)blocks, (unsigned)(n * N));
    if (is_uint8) {
      if (vec) hipLaunchKernelGGL((vitenc::vit_patch_rows_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
      else hipLaunchKernelGGL((vitenc::vit_patch_rows_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
      if (vec) hipLaunchKernelGGL((vitenc::vit_patch_rows_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
      else hipLaunchKernelGGL((vitenc::vit_patch_rows_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    if (const int rc = check_launch("ifx_vit_patch_rows")) return rc;
  }
  return IFX_OK;
}

extern "C" int ifx_vit_latent_head(const ifx_bf16* x, int32_t ldx, const ifx_bf16* gamma, const ifx_bf16* beta, const ifx_bf16* weight,
                                   const ifx_bf16* bias, ifx_bf16* out, int64_t out_batch_stride, int32_t batch, int32_t rows_per_tile,
                                   int32_t cls_tokens, int32_t dim, int32_t channels, int32_t store_channels, int32_t norm_code, float eps,
                                   void* stream) {
  IFX_REQUIRE(x && gamma && beta && weight && bias && out, "ifx_vit_latent_head: null argument");
  IFX_REQUIRE(batch >= 1 && rows_per_tile >= 1, "ifx_vit_latent_head: empty batch (%d) / rows_per_tile (%d)", batch, rows_per_tile);
  IFX_REQUIRE(cls_tokens >= 0 && cls_tokens < rows_per_tile, "ifx_vit_latent_head: cls_tokens (%d) outside [0, rows_per_tile %d)", cls_tokens,
              rows_per_tile);
  IFX_REQUIRE(dim >= 8 && channels >= 1, "ifx_vit_latent_head: dim (%d) must be >= 8, channels (%d) >= 1", dim, channels);
  if (dim % 8 != 0 || dim > 1024 || channels > 32) {
    set_error("ifx_vit_latent_head: dim %d x channels %d not built (dim a multiple of 8 up to 1024, up to 32 channels)", dim, channels);
    return IFX_EUNSUP;
  }
  IFX_REQUIRE(store_channels >= 1 && store_channels <= channels, "ifx_vit_latent_head: store_channels (%d) outside [1, channels %d]",
              store_channels, channels);
  IFX_REQUIRE(ldx % 8 == 0 && ldx >= dim, "ifx_vit_latent_head: ldx (%d) must be a multiple of 8 and >= dim (%d)", ldx, dim);
  const long long tokens = rows_per_tile - cls_tokens;
  IFX_REQUIRE(out_batch_stride >= (long long)store_channels * tokens,
              "ifx_vit_latent_head: out_batch_stride (%lld) is smaller than %d channels x %lld tokens", (long long)out_batch_stride,
              store_channels, tokens);
  IFX_REQUIRE(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)weight) % 16 == 0 && ((uintptr_t)out | (uintptr_t)bias) % 2 == 0,
              "ifx_vit_latent_head: x, gamma, beta and weight must be 16-byte aligned, bias and out 2-byte aligned");
  vitenc::HeadArgs a;
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.w = weight;
  a.bias = bias;
  a.out = out;
  a.out_stride = out_batch_stride;
  a.rows = (long long)batch * rows_per_tile;
  a.ld = ldx;
  a.D = dim;
  a.C2 = channels;
  a.store = store_channels;
  a.rows_per_tile = rows_per_tile;
  a.cls = cls_tokens;
  a.norm_code = norm_code != 0;
  a.eps = eps;
  const int dev = current_device();
  const long long want = (a.rows + 3) / 4;
  const int blocks = (int)std::min<long long>(want, 2LL * device_cu_count(dev));      // two 64 KiB workgroups fit a CU's LDS
  const int lds = channels * dim * 2;
  const dim3 grid((unsigned)blocks), block(256);
  int rc;
  if (dim <= 512) {
    rc = channels <= 8 ? launch_lds_on<vitenc::vit_latent_head_kernel<1, 8>>(dev, grid, block, lds, (hipStream_t)stream, "ifx_vit_latent_head", a)
                       : launch_lds_on<vitenc::vit_latent_head_kernel<1, 32>>(dev, grid, block, lds, (hipStream_t)stream, "ifx_vit_latent_head", a);
  } else {
    rc = channels <= 8 ? launch_lds_on<vitenc::vit_latent_head_kernel<2, 8>>(dev, grid, block, lds, (hipStream_t)stream, "ifx_vit_latent_head", a)
                       : launch_lds_on<vitenc::vit_latent_head_kernel<2, 32>>(dev, grid, block, lds, (hipStream_t)stream, "ifx_vit_latent_head", a);
  }
  if (rc) return rc;
  return check_launch("ifx_vit_latent_head");
}

extern "C" int ifx_vit_latent_blend(ifx_bf16* arena, int64_t arena_elements, const int64_t* table, const int64_t* max_tile_elements,
                                    int32_t planes, int32_t tiles_t, int32_t tiles_h, int32_t tiles_w, int32_t blend_t, int32_t blend_h,
                                    int32_t blend_w, void* stream) {
  IFX_REQUIRE(arena && table && max_tile_elements, "ifx_vit_latent_blend: null arena / table / max_tile_elements");
  IFX_REQUIRE(arena_elements >= 1 && planes >= 1, "ifx_vit_latent_blend: arena_elements (%lld) and planes (%d) must be >= 1",
              (long long)arena_elements, planes);
  IFX_REQUIRE(tiles_t >= 1 && tiles_h >= 1 && tiles_w >= 1 && (long long)tiles_t * tiles_h * tiles_w <= 65535,
              "ifx_vit_latent_blend: tile grid %d x %d x %d (1 .. 65535 tiles)", tiles_t, tiles_h, tiles_w);
  IFX_REQUIRE(blend_t >= 0 && blend_h >= 0 && blend_w >= 0, "ifx_vit_latent_blend: blend extents (%d, %d, %d) must be >= 0", blend_t, blend_h,
              blend_w);
  IFX_REQUIRE((uintptr_t)table % 8 == 0 && (uintptr_t)arena % 2 == 0, "ifx_vit_latent_blend: table must be 8-byte, arena 2-byte aligned");
  vitenc::LatentBlendArgs a;
  a.arena = arena;
  a.tab = (const long long*)table;
  a.arena_elements = arena_elements;
  a.nc = planes;
  a.nt = tiles_t;
  a.nh = tiles_h;
  a.nw = tiles_w;
  a.et = blend_t;
  a.eh = blend_h;
  a.ew = blend_w;
  // tiles of diagonal d sit behind each other in the table's id list; d = 0 is tile (0, 0, 0), which has no neighbour
  const int diagonals = tiles_t + tiles_h + tiles_w - 2;
  for (int d = 0; d < diagonals; ++d)
    IFX_REQUIRE(max_tile_elements[d] >= 1 && max_tile_elements[d] <= arena_elements,
                "ifx_vit_latent_blend: diagonal %d: max_tile_elements %lld outside [1, arena %lld]", d, (long long)max_tile_elements[d],
                (long long)arena_elements);
  int first = 0;
  for (int d = 0; d < diagonals; ++d) {
    int count = 0;
    for (int f = 0; f < tiles_t; ++f)
      for (int i = 0; i < tiles_h; ++i) {
        const int j = d - f - i;
        count += j >= 0 && j < tiles_w;
      }
    const long long biggest = max_tile_elements[d];
    if (d > 0) {
      a.first = first;
      const dim3 grid((unsigned)((biggest + 255) / 256), (unsigned)count);
      hipLaunchKernelGGL(vitenc::vit_latent_blend_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
      if (const int rc = check_launch("ifx_vit_latent_blend")) return rc;
    }
    first += count;
  }
  return IFX_OK;
}

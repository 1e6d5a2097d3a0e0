// Frame finishing of the streaming path, gfx950 only: the decoder's bf16 pixels in [-1, 1] -> the uint8 frames a consumer gets.
//
// Replaces the fp32 chain that followed every decoded block — `decode_to_pixel(...).float().clamp_(-1, 1)` (wrapper.py:160-166),
// `(v * 0.5 + 0.5).clamp(0, 1)` and `clamp(frames * 255, 0, 255).to(uint8)` (pipeline/self_forcing/pipeline.py:700-730): six
// elementwise passes over an fp32 copy of the block (4 + 4 bytes per element each) become one pass of 2 bytes in, 1 byte out.  The
// decoder's head convolution already writes `[t, h, w, 3]`, which is the frame layout, so the op is flat over the elements.
//
// Memory-bound: a lane loads 16 bytes (8 pixels' worth of bf16) and stores 8 bytes per iteration of a grid-stride loop.  The loads
// are aligned by a scalar head of up to 7 elements; where that leaves the stores 8-byte aligned as well (always, for the decoder's
// own buffers) they are one 8-byte store per lane, otherwise eight single bytes.  A scalar tail takes the last n % 8 elements.
#include "ifx_common.h"

namespace ifx {
namespace frames {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;      // 4 workgroups = 16 waves per CU on 256 CUs; longer inputs go round the grid-stride loop

// every operation is the fp32 operation torch runs at that point of the chain; f * 0.5f is exact, so a contracted fma changes nothing
__device__ __forceinline__ unsigned int to_u8(unsigned short u) {
  float f = bf2f(u);
  f = fminf(fmaxf(f, -1.0f), 1.0f);
  float g = f * 0.5f + 0.5f;
  g = fminf(fmaxf(g, 0.0f), 1.0f);
  const float h = fminf(fmaxf(g * 255.0f, 0.0f), 255.0f);
  return (unsigned int)(int)h;                      // truncation, as `.to(torch.uint8)`
}

template <bool VEC_STORE>
__global__ __launch_bounds__(kBlock) void frames_u8_kernel(const unsigned short* __restrict__ x, unsigned char* __restrict__ y,
                                                           long long n, int head) {
  const long long nvec = (n - head) >> 3;
  const u16x8* xv = reinterpret_cast<const u16x8*>(x + head);
  unsigned char* yb = y + head;
  const long long step = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += step) {
    const u16x8 v = xv[i];
    unsigned int p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = to_u8(v[k]);
    if (VEC_STORE) {
      u32x2 o;
      o[0] = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
      o[1] = p[4] | (p[5] << 8) | (p[6] << 16) | (p[7] << 24);
      *reinterpret_cast<u32x2*>(yb + 8 * i) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) yb[8 * i + k] = (unsigned char)p[k];
    }
  }
  if (blockIdx.x == 0) {                            // scalar head (lanes 0 .. 7) and tail (lanes 64 .. 71) of the first workgroup
    const int t = threadIdx.x;
    if (t < head) y[t] = (unsigned char)to_u8(x[t]);
    const long long e = head + 8 * nvec + (t - 64);
    if (t >= 64 && t < 72 && e < n) y[e] = (unsigned char)to_u8(x[e]);
  }
}

}  // namespace frames

// YUV 4:2:0 finishing (ifx_frames_yuv420, ifx_rgb8_yuv420): the same uint8 R, G, B as above (or uint8 input as it is) -> a Y plane and
// box-filtered chroma, in the integer arithmetic of include/inferix_hip.h, so that every byte is defined.  Memory-bound, no LDS.  The
// vector kernel gives a lane 2 rows x 8 columns: per row three 16-byte loads (bf16) or three 8-byte loads (uint8), out go two 8-byte Y
// stores and 4 + 4 bytes of U and V (i420) or 8 bytes of interleaved UV (nv12).  It needs w % 8 == 0, x aligned to its loads and y to
// 8 bytes, which then holds for every row and plane of every frame.  The general kernel gives a lane one 2 x 2 quad with scalar
// accesses: any even w, any alignment.  Both walk a capped grid.
namespace yuv {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;      // as frames::kMaxBlocks; more units go round the grid-stride loop

__device__ __forceinline__ unsigned int chan(unsigned short u) { return frames::to_u8(u); }
__device__ __forceinline__ unsigned int chan(unsigned char u) { return u; }

// row `r` of the descriptor on one (averaged) pixel: clamp255((m . rgb + a) >> 8), evaluated as clamp(m . rgb + a, 0, 65535) >> 8, which
// is the same number.  Why this form and not shift-then-clamp: profiles/r24_yuv420.md, "One observation on the way".
__device__ __forceinline__ unsigned int mix(const ifx_yuv420_desc& c, int r, unsigned int red, unsigned int green, unsigned int blue) {
  const int s = c.m[3 * r] * (int)red + c.m[3 * r + 1] * (int)green + c.m[3 * r + 2] * (int)blue + c.a[r];
  return (unsigned int)min(max(s, 0), 65535) >> 8;
}

// 8 pixels = 24 channel values of one row, from 48 (bf16) or 24 (uint8) aligned bytes
__device__ __forceinline__ void load_row(const unsigned short* p, unsigned int (&v)[24]) {
  const u16x8* q = reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const u16x8 e = q[j];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[8 * j + k] = chan((unsigned short)e[k]);
  }
}
__device__ __forceinline__ void load_row(const unsigned char* p, unsigned int (&v)[24]) {
  const u32x2* q = reinterpret_cast<const u32x2*>(p);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const u32x2 e = q[j];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[8 * j + k] = (e[k >> 2] >> (8 * (k & 3))) & 255u;
  }
}

__device__ __forceinline__ unsigned int pack4(unsigned int a, unsigned int b, unsigned int c, unsigned int d) {
  return a | (b << 8) | (c << 16) | (d << 24);
}

// units: t * (h / 2) row pairs of w / 8 column groups; the input is contiguous over frames, so its address needs the row pair only
template <typename IN>
__global__ __launch_bounds__(kBlock) void yuv420_vec_kernel(const IN* __restrict__ x, unsigned char* __restrict__ y, unsigned int units,
                                                            int h, int w, int nv12, ifx_yuv420_desc c) {
  const unsigned int wq = (unsigned int)w >> 3, hh = (unsigned int)h >> 1;
  const long long plane = (long long)h * w, row = (long long)w * 3;
  const unsigned int step = gridDim.x * kBlock;
  for (unsigned int i = blockIdx.x * kBlock + threadIdx.x; i < units; i += step) {
    const unsigned int rp = i / wq, qx = i - rp * wq;
    const unsigned int f = rp / hh, qy = rp - f * hh;
    unsigned int a[24], b[24];
    const IN* src = x + (long long)rp * 2 * row + 24 * qx;
    load_row(src, a);
    load_row(src + row, b);
    unsigned char* yf = y + (long long)f * (plane + (plane >> 1));
    unsigned char* y0 = yf + (long long)(2 * qy) * w + 8 * qx;
    unsigned int ya[8], yb[8], u[4], v[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ya[k] = mix(c, 0, a[3 * k], a[3 * k + 1], a[3 * k + 2]);
      yb[k] = mix(c, 0, b[3 * k], b[3 * k + 1], b[3 * k + 2]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned int red = (a[6 * k] + a[6 * k + 3] + b[6 * k] + b[6 * k + 3] + 2) >> 2;
      const unsigned int green = (a[6 * k + 1] + a[6 * k + 4] + b[6 * k + 1] + b[6 * k + 4] + 2) >> 2;
      const unsigned int blue = (a[6 * k + 2] + a[6 * k + 5] + b[6 * k + 2] + b[6 * k + 5] + 2) >> 2;
      u[k] = mix(c, 1, red, green, blue);
      v[k] = mix(c, 2, red, green, blue);
    }
    u32x2 o;
    o[0] = pack4(ya[0], ya[1], ya[2], ya[3]);
    o[1] = pack4(ya[4], ya[5], ya[6], ya[7]);
    *reinterpret_cast<u32x2*>(y0) = o;
    o[0] = pack4(yb[0], yb[1], yb[2], yb[3]);
    o[1] = pack4(yb[4], yb[5], yb[6], yb[7]);
    *reinterpret_cast<u32x2*>(y0 + w) = o;
    if (nv12) {
      o[0] = pack4(u[0], v[0], u[1], v[1]);
      o[1] = pack4(u[2], v[2], u[3], v[3]);
      *reinterpret_cast<u32x2*>(yf + plane + (long long)qy * w + 8 * qx) = o;
    } else {
      unsigned char* up = yf + plane + (long long)qy * (w >> 1) + 4 * qx;
      *reinterpret_cast<unsigned int*>(up) = pack4(u[0], u[1], u[2], u[3]);
      *reinterpret_cast<unsigned int*>(up + (plane >> 2)) = pack4(v[0], v[1], v[2], v[3]);
    }
  }
}

// units: t * (h / 2) * (w / 2) quads
template <typename IN>
__global__ __launch_bounds__(kBlock) void yuv420_quad_kernel(const IN* __restrict__ x, unsigned char* __restrict__ y, unsigned int units,
                                                             int h, int w, int nv12, ifx_yuv420_desc c) {
  const unsigned int wh = (unsigned int)w >> 1, hh = (unsigned int)h >> 1;
  const long long plane = (long long)h * w, row = (long long)w * 3;
  const unsigned int step = gridDim.x * kBlock;
  for (unsigned int i = blockIdx.x * kBlock + threadIdx.x; i < units; i += step) {
    const unsigned int rp = i / wh, qx = i - rp * wh;
    const unsigned int f = rp / hh, qy = rp - f * hh;
    const IN* src = x + (long long)rp * 2 * row + 6 * qx;
    unsigned int p[2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 6; ++k) p[r][k] = chan(src[r * row + k]);
    unsigned char* yf = y + (long long)f * (plane + (plane >> 1));
    unsigned char* y0 = yf + (long long)(2 * qy) * w + 2 * qx;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      y0[(long long)r * w] = (unsigned char)mix(c, 0, p[r][0], p[r][1], p[r][2]);
      y0[(long long)r * w + 1] = (unsigned char)mix(c, 0, p[r][3], p[r][4], p[r][5]);
    }
    const unsigned int red = (p[0][0] + p[0][3] + p[1][0] + p[1][3] + 2) >> 2;
    const unsigned int green = (p[0][1] + p[0][4] + p[1][1] + p[1][4] + 2) >> 2;
    const unsigned int blue = (p[0][2] + p[0][5] + p[1][2] + p[1][5] + 2) >> 2;
    const unsigned char u = (unsigned char)mix(c, 1, red, green, blue), v = (unsigned char)mix(c, 2, red, green, blue);
    if (nv12) {
      unsigned char* uv = yf + plane + (long long)qy * w + 2 * qx;
      uv[0] = u;
      uv[1] = v;
    } else {
      unsigned char* up = yf + plane + (long long)qy * wh + qx;
      up[0] = u;
      up[plane >> 2] = v;
    }
  }
}

template <typename IN>
int launch(const char* name, const IN* x, uint8_t* y, int t, int h, int w, int layout, const ifx_yuv420_desc* coeffs, void* stream) {
  IFX_REQUIRE(x && y && coeffs, "%s: null argument", name);
  IFX_REQUIRE(t >= 0 && h >= 0 && w >= 0, "%s: negative size (t %d, h %d, w %d)", name, t, h, w);
  IFX_REQUIRE((h & 1) == 0 && (w & 1) == 0, "%s: 4:2:0 needs an even frame size, got h %d, w %d", name, h, w);
  IFX_REQUIRE(layout == IFX_YUV420_I420 || layout == IFX_YUV420_NV12, "%s: unknown layout %d (IFX_YUV420_I420 0, IFX_YUV420_NV12 1)",
              name, layout);
  IFX_REQUIRE(((uintptr_t)x & (sizeof(IN) - 1)) == 0, "%s: x must be %d-byte aligned", name, (int)sizeof(IN));
  if (t == 0 || h == 0 || w == 0) return IFX_OK;
  const long long quads = (long long)t * (h >> 1) * (w >> 1);
  IFX_REQUIRE(quads <= 0x7fffffffLL, "%s: launch too large (%d frames of %d x %d)", name, t, h, w);
  const bool vec = (w & 7) == 0 && ((uintptr_t)x & (8 * sizeof(IN) - 1)) == 0 && ((uintptr_t)y & 7) == 0;
  const unsigned int units = (unsigned int)(vec ? quads >> 2 : quads);
  unsigned int blocks = (units + kBlock - 1) / kBlock;
  blocks = blocks > (unsigned int)kMaxBlocks ? (unsigned int)kMaxBlocks : blocks;
  if (vec)
    hipLaunchKernelGGL(yuv420_vec_kernel<IN>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, units, h, w, layout, *coeffs);
  else
    hipLaunchKernelGGL(yuv420_quad_kernel<IN>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, units, h, w, layout, *coeffs);
  return check_launch(name);
}

}  // namespace yuv
}  // namespace ifx

using namespace ifx;

extern "C" int ifx_frames_yuv420(const ifx_bf16* x, uint8_t* y, int32_t t, int32_t h, int32_t w, int32_t layout,
                                 const ifx_yuv420_desc* coeffs, void* stream) {
  return yuv::launch("ifx_frames_yuv420", reinterpret_cast<const unsigned short*>(x), y, t, h, w, layout, coeffs, stream);
}

extern "C" int ifx_rgb8_yuv420(const uint8_t* x, uint8_t* y, int32_t t, int32_t h, int32_t w, int32_t layout,
                               const ifx_yuv420_desc* coeffs, void* stream) {
  return yuv::launch("ifx_rgb8_yuv420", x, y, t, h, w, layout, coeffs, stream);
}

extern "C" int ifx_frames_u8(const ifx_bf16* x, uint8_t* y, int64_t n, void* stream) {
  IFX_REQUIRE(x && y, "ifx_frames_u8: null argument");
  IFX_REQUIRE(n >= 0, "ifx_frames_u8: negative element count %lld", (long long)n);
  IFX_REQUIRE(((uintptr_t)x & 1) == 0, "ifx_frames_u8: x must be 2-byte aligned");
  if (n == 0) return IFX_OK;
  int head = (int)(((16 - ((uintptr_t)x & 15)) & 15) >> 1);            // elements in front of the first 16-byte aligned load
  if (head > n) head = (int)n;
  const long long nvec = ((long long)n - head) >> 3;
  long long blocks = (nvec + frames::kBlock - 1) / frames::kBlock;
  blocks = blocks < 1 ? 1 : (blocks > frames::kMaxBlocks ? frames::kMaxBlocks : blocks);
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(x);
  if ((((uintptr_t)y + head) & 7) == 0)
    hipLaunchKernelGGL(frames::frames_u8_kernel<true>, dim3((unsigned)blocks), dim3(frames::kBlock), 0, (hipStream_t)stream, xs, y,
                       (long long)n, head);
  else
    hipLaunchKernelGGL(frames::frames_u8_kernel<false>, dim3((unsigned)blocks), dim3(frames::kBlock), 0, (hipStream_t)stream, xs, y,
                       (long long)n, head);
  return check_launch("ifx_frames_u8");
}

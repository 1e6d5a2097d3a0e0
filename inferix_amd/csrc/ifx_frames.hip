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
}  // namespace ifx

using namespace ifx;

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

// The host-side decisions of ifx_conv.hip, ONCE: what ifx_conv3d_cl refuses, which kernel it launches (lock-step or persistent
// ping-pong), on which channel tile, over how many tiles, with how much dynamic LDS and on which grid; and the (G, CPL, blocks) rule of
// ifx_rmsnorm_cl.  The LDS geometry of the two conv kernels (Geo, GeoP) lives here as well: it is constexpr only, the kernels read
// their offsets from it and the plan reads its LDS bytes from it, so the two cannot drift.  Host only: no kernels, no GPU calls, no HIP
// header — tools/conv_plan_check.cpp runs every decision without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/inferix_hip.h"

namespace ifx {
void set_error(const char* fmt, ...);      // ifx_core.hip
}
#ifndef IFX_REQUIRE      // as in ifx_common.h, which needs the HIP headers
#define IFX_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ifx::set_error(__VA_ARGS__);        \
      return IFX_EINVAL;                  \
    }                                     \
  } while (0)
#endif

namespace ifx {
namespace conv {

constexpr int TH = 8, TW = 64;          // output tile (pixels)
constexpr int MAXF = 16;                // frames per call (inputs incl. history / outputs)

#ifndef IFX_CONV_LOADER_WAVES
#define IFX_CONV_LOADER_WAVES 4
#endif

template <int BN, int UPS, int KS>
struct Geo {
  static constexpr int TAPS = KS * KS;
  static constexpr int TG = TAPS == 9 ? 3 : 1;          // taps per barrier interval ("group" = one kernel row)
  static constexpr int GPS = TAPS / TG;                 // groups per stage
  static constexpr int PH = UPS ? TH / 2 + 2 : TH + KS - 1;
  static constexpr int PW = UPS ? TW / 2 + 2 : TW + KS - 1;
  static constexpr int NP = PH * PW;                    // patch pixels
  static constexpr int NPI = (NP + 15) / 16;            // 1 KiB DMA instructions per patch
  // LDS-DMA costs its issuing wave ~65 cycles per instruction and is serialised per SIMD, but does not hold back the other
  // wave of the SIMD (tools/probe_overlap.hip): only waves 0 .. LW-1 (the older wave of each SIMD) issue DMA, the younger
  // ones go straight to the matrix pipe after the barrier.
  static constexpr int LW = IFX_CONV_LOADER_WAVES;
  static constexpr int PPW = (NPI + LW - 1) / LW;       // patch pieces per loader wave
  static constexpr int P_SLOT = NPI * 1024;
  static constexpr int WP = BN / 16;                    // 1 KiB weight pieces per tap (16 rows x 32 channels)
  static constexpr int W_TAP = BN * 64;
  static constexpr int WPW = (TG * WP + LW - 1) / LW;    // weight pieces per loader wave per group
  static constexpr int WRG = TAPS == 9 ? (BN == 128 ? 2 : 3) : 2;   // weight ring depth in groups
  static constexpr int L = WRG - 1;                     // groups of weight lookahead
  static constexpr int P_OFF = 0, W_OFF = 2 * P_SLOT, S_OFF = W_OFF + WRG * TG * W_TAP, LDS_MAIN = S_OFF + LW * 1024;
  static constexpr int LDS_EPI = 8 * 64 * (BN * 2 + 16);      // per-wave transpose regions of the epilogue (reuse the rings)
  static constexpr int LDS = LDS_MAIN > LDS_EPI ? LDS_MAIN : LDS_EPI;
  static constexpr bool PF = BN <= 96;                  // fragments of the next tap prefetched under the MFMAs of this one
  static_assert(L == 1 || GPS >= 3, "patch of the next stage is issued in group 0 and must precede weights two groups on");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

namespace pp {
template <int BN, int UPS>
struct GeoP {
  static constexpr int PH = UPS ? TH / 2 + 2 : TH + 2, PW = UPS ? TW / 2 + 2 : TW + 2;
  static constexpr int NP = PH * PW, NPI = (NP + 15) / 16;
  // a stage's NPI patch pieces: group 0 moves the first 4 * PG0 (one per wave in each of its loader phases 6t-1, 6t+1, 6t+3: its loader
  // phases carry the 4-5 weight pieces per wave, ~90 cycles each, and a patch piece costs ~300 — 64-byte rows 192+ bytes apart), group 1
  // the rest in two batches (loader phases 6t, 6t+2)
  static constexpr int PG0 = UPS ? 1 : 3;               // (1 or 2 for the plain kernel: group 1's lane terms no longer fit, 1-3 registers spill)
  static constexpr int NP1 = NPI - 4 * PG0;
  static constexpr int PPW = (NP1 + 3) / 4;             // patch piece slots per wave of group 1 and stage
  static constexpr int QA = (PPW + 1) / 2;              // of which in the first of the stage's two batches
  static constexpr int P_SLOT = NPI * 1024;
  static constexpr int WP = BN / 16;                    // 1 KiB weight pieces per tap
  static constexpr int W_TAP = BN * 64, W_STEP = 3 * W_TAP;
  static constexpr int WPS = 3 * WP, WPW = (WPS + 3) / 4;      // weight pieces per step / piece slots per wave of group 0 and step
  static constexpr int PITCH = BN * 2 + 16, SCR = 32 * PITCH;  // transpose region of one wave: 32 pixels x BN channels
  static constexpr int P_OFF = 0, W_OFF = 2 * P_SLOT, E_OFF = W_OFF + 2 * W_STEP;
  static constexpr int B_OFF = E_OFF + 4 * SCR;         // the launch's bias vector (Cout <= 512 channels) as bf16
  static constexpr int S_OFF = B_OFF + 1024;            // 256-byte sinks of the residual warm-up requests, one per wave
  static constexpr int LDS = S_OFF + 8 * 256;
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static_assert(SCR % 16 == 0 && P_SLOT % 16 == 0 && W_STEP % 16 == 0, "alignment");
};
}  // namespace pp

// ---- the instantiations of the two conv kernels: what ifx_conv.hip builds and launches from, row by row
enum ConvKernel : int { kConvLockStep, kConvPersistent };      // conv_cl_kernel<bn, ups, ks> / pp::conv_pp_kernel<bn, ups> (3 x 3 only)
struct ConvShape {
  ConvKernel kind;
  int bn, ups, ks, lds;
};
template <int BN, int UPS, int KS>
constexpr ConvShape lock_step() { return {kConvLockStep, BN, UPS, KS, Geo<BN, UPS, KS>::LDS}; }
template <int BN, int UPS>
constexpr ConvShape persistent() { return {kConvPersistent, BN, UPS, 3, pp::GeoP<BN, UPS>::LDS}; }
constexpr ConvShape kConvShapes[] = {
    lock_step<32, 0, 1>(), lock_step<64, 0, 1>(), lock_step<96, 0, 1>(), lock_step<128, 0, 1>(),
    lock_step<32, 0, 3>(), lock_step<64, 0, 3>(), lock_step<96, 0, 3>(), lock_step<128, 0, 3>(),
    lock_step<32, 1, 3>(), lock_step<64, 1, 3>(), lock_step<96, 1, 3>(), lock_step<128, 1, 3>(),
    persistent<96, 0>(),   persistent<96, 1>(),
};
constexpr int kConvShapeCount = sizeof(kConvShapes) / sizeof(kConvShapes[0]);

struct ConvPlan : ConvShape {                        // the row of kConvShapes that runs
  int shape;                                         // its index
  int ho, wo;                                        // output frame
  int tiles_w, tiles_h, tiles_n, total, per_xcd;     // TH x TW x bn tiles; all of them over t_out frames; per XCD (eight of them)
  // workgroups: the lock-step kernel one per tile, rounded up to the same number on every XCD (whatever `cus`); the persistent kernel
  // one per CU (LDS), the same number on every XCD, and no more than an XCD has tiles
  int grid(int cus) const {
    const int wgx = kind == kConvLockStep || per_xcd < cus / 8 ? per_xcd : cus / 8;
    return (wgx > 1 ? wgx : 1) * 8;
  }
};

// Every argument check of ifx_conv3d_cl (IFX_EINVAL with the entry point's texts), then the plan of the launch.  `variant`: conv_variant.
static inline int conv_plan(const ifx_conv3d_desc& d, int variant, ConvPlan& p) {
  IFX_REQUIRE(d.x && d.w && d.y && d.zero_page, "ifx_conv3d_cl: null argument");
  IFX_REQUIRE(d.kt == 1 || d.kt == 3, "ifx_conv3d_cl: temporal kernel %d not built (1 or 3)", d.kt);
  IFX_REQUIRE(d.ks == 1 || d.ks == 3, "ifx_conv3d_cl: spatial kernel %d not built (1 or 3)", d.ks);
  IFX_REQUIRE(d.upsample == 0 || (d.upsample == 1 && d.ks == 3), "ifx_conv3d_cl: upsample needs the 3x3 kernel");
  IFX_REQUIRE(d.cin > 0 && d.cin % 32 == 0, "ifx_conv3d_cl: cin %d must be a multiple of 32", d.cin);
  IFX_REQUIRE(d.in_planar == 0 || d.in_planar == 1, "ifx_conv3d_cl: in_planar %d (0 or 1)", d.in_planar);
  IFX_REQUIRE(d.cout > 0 && (d.cout % 4 == 0 || d.cout < 4), "ifx_conv3d_cl: cout %d must be a multiple of 4 (or < 4)", d.cout);
  IFX_REQUIRE(d.t_out >= 1 && d.t_out + d.kt - 1 <= MAXF, "ifx_conv3d_cl: %d output frames per call (max %d inputs)", d.t_out, MAXF);
  IFX_REQUIRE(d.hs > 0 && d.ws > 0, "ifx_conv3d_cl: empty frame");
  p.ho = d.hs << d.upsample;
  p.wo = d.ws << d.upsample;
  const long long in_frame = (long long)d.hs * d.ws * d.cin, out_frame = (long long)p.ho * p.wo * d.cout;      // elements
  const long long weights = (long long)d.kt * d.ks * d.ks * d.cin * d.cout;
  IFX_REQUIRE(in_frame < (1ll << 31) && out_frame < (1ll << 31), "ifx_conv3d_cl: frame too large for 32-bit pixel offsets");
  // both kernels move 16 bytes per lane: LDS-DMA from x and w whatever the shape; whole-pixel stores to y and residual loads where
  // cout % 8 == 0 (other channel counts are stored and read element by element)
  const auto misaligned = [](const void* ptr) { return ((uintptr_t)ptr & 15) != 0; };
  IFX_REQUIRE(d.in_frame_stride % 8 == 0, "ifx_conv3d_cl: in_frame_stride %lld must be a multiple of 8 elements (16 bytes)",
              (long long)d.in_frame_stride);
  IFX_REQUIRE(!misaligned(d.x) && !misaligned(d.w), "ifx_conv3d_cl: x and w must be 16-byte aligned");
  if (d.cout % 8 == 0) {
    IFX_REQUIRE(d.out_frame_stride % 8 == 0, "ifx_conv3d_cl: out_frame_stride %lld must be a multiple of 8 elements (16 bytes) when cout %% 8 == 0",
                (long long)d.out_frame_stride);
    IFX_REQUIRE(!misaligned(d.y) && !misaligned(d.residual), "ifx_conv3d_cl: y and residual must be 16-byte aligned when cout %% 8 == 0");
  }
  // channel tile: 96 wherever it divides (fragment prefetch + two weight groups ahead fit the register / LDS budget,
  // and 384 = 4 x 96 gives the 60 x 104 level more workgroups), else 128 / 64 / 32
  const int bn = d.cout <= 32 ? 32 : d.cout % 96 == 0 ? 96 : d.cout % 128 == 0 ? 128 : d.cout <= 64 ? 64 : 128;
  // the persistent ping-pong kernel serves the 3 x 3 spatial kernels on 96-channel tiles (every expensive layer of the decoder) unless
  //   * option conv_variant = 1 keeps the lock-step kernel (A/B, tools/bench_vae.py --variant);
  //   * cout > 512: its copy of the launch's bias vector in LDS is 1 KiB;
  //   * an input frame, an output frame or the weights take 2 GiB or more: it addresses each through one buffer descriptor with
  //     signed 32-bit BYTE offsets (the lock-step kernel adds 32-bit ELEMENT offsets of a pixel to 64-bit frame / tap bases).
  const long long two_gib = 1ll << 31;
  const bool persistent_fits = d.cout <= 512 && in_frame * 2 < two_gib && out_frame * 2 < two_gib && weights * 2 < two_gib;
  const ConvKernel kind = d.ks == 3 && bn == 96 && variant != 1 && persistent_fits ? kConvPersistent : kConvLockStep;
  p.shape = -1;
  for (int i = 0; i < kConvShapeCount && p.shape < 0; ++i) {
    const ConvShape& s = kConvShapes[i];
    if (s.kind == kind && s.bn == bn && s.ups == d.upsample && s.ks == d.ks) static_cast<ConvShape&>(p) = s, p.shape = i;
  }
  if (p.shape < 0) {      // (no valid call gets here: every (bn, upsample, ks) above has its lock-step row)
    set_error("ifx_conv3d_cl: no kernel for a %d-channel tile, spatial kernel %d, upsample %d", bn, d.ks, d.upsample);
    return IFX_EUNSUP;
  }
  p.tiles_w = (p.wo + TW - 1) / TW;
  p.tiles_h = (p.ho + TH - 1) / TH;
  p.tiles_n = (d.cout + p.bn - 1) / p.bn;
  p.total = p.tiles_w * p.tiles_h * p.tiles_n * d.t_out;
  p.per_xcd = (p.total + 7) / 8;
  return IFX_OK;
}

// ---- ifx_rmsnorm_cl: G lanes (a power of two) share one pixel and hold CPL 16-byte chunks of it each: CPL = 3 where a third of the
// chunks is a power of two (the decoder's 96 / 192 / 384 channels: every lane busy), else CPL = 1 and G the next power of two.  A block
// of 256 lanes takes 256 / G groups x NPX pixels, NPX = 4 (CPL 1) or 2 (CPL 3) as in rmsnorm_cl_kernel.
constexpr int kNormShapes[][2] = {{1, 1}, {2, 1}, {4, 1}, {8, 1}, {16, 1}, {32, 1}, {64, 1},      // (G, CPL): the instantiations built
                                  {1, 3}, {2, 3}, {4, 3}, {8, 3}, {16, 3}, {32, 3}, {64, 3}};
constexpr int kNormShapeCount = sizeof(kNormShapes) / sizeof(kNormShapes[0]);
struct NormPlan {
  int g, cpl;
  long long blocks;
};
static inline NormPlan norm_plan(int channels, long long pixels) {      // channels in [8, 512] step 8 (checked by the entry point)
  const int chunks = channels / 8;
  const bool thirds = chunks % 3 == 0 && (chunks / 3 & (chunks / 3 - 1)) == 0;
  NormPlan p = {1, thirds ? 3 : 1, 0};
  while (p.g * p.cpl < chunks) p.g *= 2;
  const long long per_block = (256 / p.g) * (p.cpl == 1 ? 4 : 2);
  p.blocks = (pixels + per_block - 1) / per_block;
  return p;
}

}  // namespace conv
}  // namespace ifx

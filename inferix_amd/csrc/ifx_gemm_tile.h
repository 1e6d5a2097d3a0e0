// What the LDS-DMA GEMM tiles share, ONCE: the XCD-aware grouped raster (device) and the launch sequence (host).  Users: the four
// kernel templates of ifx_gemm_glds.hip and gemm_q8_dma_kernel of ifx_quant.hip; the raster also serves the register-staged,
// four-wave and ping-pong tiles.
//
// A block of kernel text moves here only if every kernel instantiation that uses the helper compiles to the machine code it had with
// the block written out (tools/device_code_diff.py).  The operand staging, the counted vmcnt ladder, the fragment row tables and the
// LDS-transposed epilogue are NOT here: as functions they moved instructions or changed register allocation in every form tried, so
// each kernel keeps its copy.
#pragma once
#include <algorithm>

#include "ifx_gemm_epilogue.h"
#include "ifx_lds_dma.h"

namespace ifx {

// device side -----------------------------------------------------------------------------------------------------------------------

// Grouped raster: consecutive tile ids walk GM token-tiles, then the next channel-tile, then the next GM token-tiles -> the ~32
// workgroups resident on one XCD (which owns a contiguous id range: id = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3), tested against
// per_xcd and total by the kernel) form a GM x (32/GM) block of tiles sharing GM x-panels and 32/GM W-panels in its L2.  (An m-fastest
// order made every XCD touch every panel: 0.9-1.2 GB of memory-side fetches per GEMM.)  Returns the tile's first token row and channel.
struct TileOrigin { int m, n; };
template <int BM, int BN, int GM>
__device__ __forceinline__ TileOrigin tile_origin_of(int t_id, int tiles_m, int tiles_n) {
  const int grp_sz = GM * tiles_n;
  const int first_m = (t_id / grp_sz) * GM;
  const int gm = min(GM, tiles_m - first_m);
  const int rem = t_id % grp_sz;
  return {(first_m + rem % gm) * BM, (rem / gm) * BN};
}
template <int BM, int BN, int GM>
__device__ __forceinline__ TileOrigin tile_origin(int t_id, int tiles_m, int total) {
  return tile_origin_of<BM, BN, GM>(t_id, tiles_m, total / tiles_m);
}

// host side -------------------------------------------------------------------------------------------------------------------------

// The launch of one tile of the family.  Tile names the tile kind:
//   BM, BN, THREADS, LDS (bytes of dynamic LDS), NAME (the entry point and tile kind, for every error text of the launch) and
//   kernel<EPI>, the kernel instantiation of epilogue EPI, whose arguments are (x, ldx, w, y, ldy, M, N, K, tiles_m, total, per_xcd, ea, extra...).
// The grid is the tile count rounded up to the eight XCDs (the kernel tests its id).  No runtime call besides the launch's own.
template <class Tile, class T, class Ea, class... Extra>
static inline int launch_tile(const T* x, int ldx, const T* w, unsigned short* y, int ldy, int M, int N, int K, int mode, const Ea& ea,
                              hipStream_t s, Extra... extra) {
  const int tiles_m = (M + Tile::BM - 1) / Tile::BM, tiles_n = (N + Tile::BN - 1) / Tile::BN;
  const int total = tiles_m * tiles_n, per_xcd = (total + 7) / 8;
  const dim3 grid(per_xcd * 8), block(Tile::THREADS);
  static_assert(Tile::LDS <= 160 * 1024, "LDS");
  const int rc = dispatch_epilogue(mode, Tile::NAME, [&](auto epi_c) {
    return launch_lds<Tile::template kernel<decltype(epi_c)::value>>(grid, block, (int)Tile::LDS, s, Tile::NAME, x, ldx, w, y, ldy, M, N, K, tiles_m,
                                                                     total, per_xcd, ea, extra...);
  });
  if (rc != IFX_OK) return rc;
  return check_launch(Tile::NAME);
}

}  // namespace ifx

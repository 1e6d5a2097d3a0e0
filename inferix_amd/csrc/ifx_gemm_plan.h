// The host-side decision of the GEMM family, ONCE: which launcher a call of ifx_gemm_bf16[_ws] / ifx_gemm_q8[_ws] runs, on which tile,
// with which K split and with how much of the caller's workspace.  gemm_plan / gemm_q8_plan are what the entry points launch from AND
// what ifx_gemm_workspace_bytes / ifx_gemm_q8_workspace_bytes answer from, so the two cannot drift (they had: the query once reported up
// to 75 MB of split-K scratch for launches that never touched it).  Host only: no kernels, no GPU calls — tools/gemm_plan_check.cpp
// runs the whole decision without a GPU.
#pragma once
#include "ifx_common.h"

namespace ifx {

// LDS-DMA tiles of launch_gemm_lds_dma (ifx_gemm_glds.hip).  gemm_variant - 2 IS a tile id, so the values are fixed; an id without a
// name (18, 20 ..) runs the 64 x 64 tile too.    (bench: tools/bench_kernels.py gemm M)
enum GemmTile : int {
  kTile256x128 = 0,                                              // 256x128x64, 8 waves, ping-pong
  kTile128x128 = 1,                                              // two workgroups per CU
  kTile64x64 = 2, kTile128x64 = 4,
  kTile256x256 = 3,                                              // 64-deep, two stages, 128-byte operand rows
  kTile256x128k32 = 5, kTile128x128k32 = 6,                      // the 32-deep two-per-CU / eight-wave experiments, slower than 128x128
  kTileWs256x128 = 7, kTileWs128x128 = 8,                        // warp-specialised (producer / consumer waves); 64 KiB: two per CU
  kTile256x256k32 = 9,                                           // the 32-deep four-stage predecessor of kTile256x256
  kTile64x64Kg4 = 10, kTile64x64Kg2 = 11, kTile128x128Kg2 = 12,  // K split between four / two wave groups of ONE workgroup (no workspace)
  kTile128x64s2 = 13,                                            // two stages, 48 KiB: three workgroups per CU
  kTile64x128s2 = 14, kTile64x128s3 = 15,                        // two / three stages
  kTileFourWaveDma = 16, kTileFourWave = 17,                     // four waves of 128x128 on 256x256x64: LDS-DMA / register staged (ifx_gemm_w4.hip)
  kTile256x192 = 19,
};

// ifx_set_option("gemm_variant", v), one row per v (documented for callers in include/inferix_hip.h):
//   kind : what the variant asks for;  tile : the LDS-DMA tile it forces, or the one a launch it cannot take falls to (-1: pick_tile);
//   tj   : ping-pong tile height / 64;  ks : K parts (0 = stream-K);  takes_ws : a caller's workspace may turn into a K split
enum GemmKind : int { kGemmAuto, kGemmRegStaged, kGemmLdsDma, kGemmW4SplitK, kGemmPp, kGemmPpStreamK, kGemmPpKParts };
struct GemmVariant { GemmKind kind; int tile, tj, ks; bool takes_ws; };
constexpr GemmVariant gemm_tile_row(int t) { return {kGemmLdsDma, t, 0, 1, false}; }
constexpr GemmVariant kGemmVariants[30] = {
    {kGemmAuto, -1, 0, 1, true},                 //  0 the ping-pong tiles from 2048 rows (pick_pp), else an LDS-DMA tile by shape (pick_tile)
    {kGemmRegStaged, -1, 0, 1, false},           //  1 the register-staged 128x128 kernel of ifx_gemm.hip
    gemm_tile_row(kTile256x128), gemm_tile_row(kTile128x128), gemm_tile_row(kTile64x64), gemm_tile_row(kTile256x256),            //  2 ..  5
    gemm_tile_row(kTile128x64), gemm_tile_row(kTile256x128k32), gemm_tile_row(kTile128x128k32), gemm_tile_row(kTileWs256x128),   //  6 ..  9
    gemm_tile_row(kTileWs128x128), gemm_tile_row(kTile256x256k32), gemm_tile_row(kTile64x64Kg4), gemm_tile_row(kTile64x64Kg2),   // 10 .. 13
    gemm_tile_row(kTile128x128Kg2), gemm_tile_row(kTile128x64s2), gemm_tile_row(kTile64x128s2), gemm_tile_row(kTile64x128s3),    // 14 .. 17
    gemm_tile_row(kTileFourWaveDma), gemm_tile_row(kTileFourWave),                                                             // 18, 19
    {kGemmW4SplitK, -1, 0, 2, true},             // 20 the four-wave tile with K split over two workgroups (want_w4_splitk shapes)
    gemm_tile_row(kTile256x192),                 // 21
    {kGemmPp, -1, 4, 1, true},                   // 22 the 256-token ping-pong tile (K split in two on gemm_pp_split shapes)
    {kGemmPp, -1, 3, 1, true},                   // 23 the 192-token one (same)
    {kGemmPp, -1, 2, 1, false},                  // 24 the 128-token one (never split)
    {kGemmPp, -1, 4, 1, false},                  // 25 the 256-token one without the K split
    {kGemmPpStreamK, -1, 2, 0, true},            // 26 stream-K on the 128-token tile
    {kGemmPpKParts, 25, 2, 2, true},             // 27 } lab: the 128-token tile with K split over 2 / 4 / 8 workgroups per tile, whatever
    {kGemmPpKParts, 26, 2, 4, true},             // 28 } the shape; a launch that cannot take it has always fallen to tile id variant - 2,
    {kGemmPpKParts, 27, 2, 8, true},             // 29 } i.e. to the 64 x 64 tile
};
// (IFX_GEMM_VARIANT in the environment is not range-checked: a value past the table forces tile id v - 2, a negative one the tile choice)
static inline GemmVariant gemm_variant_row(int v) {
  return v >= 0 && v < 30 ? kGemmVariants[v] : GemmVariant{kGemmLdsDma, v >= 2 ? v - 2 : -1, 0, 1, false};
}

// the alignment facts the ping-pong tiles ask about an epilogue's operands (pp_epilogue_fits)
struct PpOperands {
  bool bias8 = true, res16 = true, mod16 = true;   // 8-byte aligned bias; 16-byte aligned residual rows (pointer and ld_res % 8); gate rows
  int rows_per_group = 1 << 30;
};
// 8-byte aligned bias, 16-byte aligned residual / gate rows, and gate groups of at least `min_rows_per_group` rows (a wave's token rows)
static inline bool pp_epilogue_fits(int mode, const PpOperands& o, int min_rows_per_group) {
  const bool res = mode == IFX_EPI_RESIDUAL || mode == IFX_EPI_GATE_RES;
  return o.bias8 && (!res || o.res16) && (mode != IFX_EPI_GATE_RES || (o.mod16 && o.rows_per_group >= min_rows_per_group));
}

// what the decision is allowed to see of a call
struct GemmRequest {
  int M, N, K, mode;            // mode: the epilogue instantiation (IFX_EPI_GELU_ERF arrives as IFX_EPI_GELU_TANH)
  // 16-byte epilogue vectors are possible (N, ldy, ld_res % 8 == 0, y / residual / mod 16-byte aligned); a second destination is asked for
  bool wide_ok = true, y2 = false;
  PpOperands ops;
  int64_t ws_bytes = 0;         // workspace on offer, 0 = none
  bool qdiv = false, qdiv16 = true;   // 8-bit entry: a static output quantiser is asked for / its divisors are 16-byte aligned
};
enum GemmPath : int { kGemmPathRegStaged, kGemmPathLdsDma, kGemmPathW4, kGemmPathPp, kGemmPathRefuseY2 };
// 8-bit entry: `tile` of kGemmPathLdsDma.  128-byte operand rows with two / three stages, or the 64-byte four-stage ring they replaced
enum GemmQ8Tile : int { kQ8Tile256x256, kQ8Tile256x128, kQ8Tile256x256Rows64, kQ8Tile256x128Rows64 };
struct GemmPlan {
  GemmPath path;
  int tile = -1, tj = 0, ks = 1;   // ks: 0 = stream-K, 1 = unsplit, 2 / 4 / 8 = K parts
  int64_t ws_bytes = 0;         // workspace the launch will touch; 0 = the launcher gets a null workspace
  bool y2 = false;              // the launch carries the request's second destination
};

// workspace sizes ----------------------------------------------------------------------------------------------------------------------
// (Row invariance holds up to 1024 tiles of a launch — 43 690 rows at N = 1536, five times the largest block of the path — which is what
//  the flag page and a workspace of at most 256 MiB cover; a larger launch runs unsplit, i.e. with the other summation order.)
// Split K in two for long-K launches with few column tiles (the block's FFN down-projection, 1536 x 8960: 114 tiles of 256 x 256 for
// 256 CUs).  Depends on (N, K) ONLY: a row's summation order must not change with the number of rows in the launch.
static inline bool gemm_pp_split(int N, int K) {
  static const int min_k = lab_env_int("IFX_PP_SPLIT_MIN_K", 4096);      // lab: where the two-workgroup split starts to pay
  return K >= min_k && N <= 2048 && (K / 64) % 2 == 0;
}
// stream-K (128-token tile): one 128 KiB slot per workgroup behind the 4 KiB of flags
static inline size_t gemm_pp_stream_k_workspace_bytes() { return 4096 + (size_t)256 * 128 * 256 * 4; }
// (the split runs on the 256- or the 192-token tile — whichever needs fewer rounds, pick_pp; the tile height does not change a bit of
//  the result — so the workspace covers the larger of the two tilings: 4096 bytes of flags + one fp32 tile image per tile)
static inline size_t gemm_pp_workspace_bytes(int M, int N, int K) {
  if (!gemm_pp_split(N, K)) return 0;
  const size_t tn = (size_t)(N + 255) / 256, t4 = (size_t)((M + 255) / 256) * tn, t3 = (size_t)((M + 191) / 192) * tn;
  if (t4 > 1024) return 0;
  const size_t b4 = t4 * 256 * 256 * 4, b3 = t3 <= 1024 ? t3 * 192 * 256 * 4 : 0;
  return 4096 + (b4 > b3 ? b4 : b3);
}
// shard-sized launches (gemm_small_split): the 128-token tile with K split over `ks` workgroups per tile — 4096 bytes of flags + one
// fp32 tile image per (tile, part >= 1)
static inline size_t gemm_pp_small_workspace_bytes(int M, int N, int ks) {
  if (ks <= 1) return 0;
  const size_t tiles = (size_t)((M + 127) / 128) * ((N + 255) / 256);
  return 4096 + tiles * (size_t)(ks - 1) * 128 * 256 * 4;
}
// the four-wave 256 x 256 tile with K halves in two workgroups: arrival counters (up to 1024 tiles) in front, then the partials
static inline size_t gemm_w4_workspace_bytes(int M, int N, int splits) {
  if (splits <= 1) return 0;
  const size_t tiles = (size_t)((M + 255) / 256) * ((N + 255) / 256);
  return 4096 + tiles * (size_t)splits * 256 * 256 * 4;
}

// the pickers ----------------------------------------------------------------------------------------------------------------------------
// The rounds model of the ping-pong tiles, fitted to tools/gemm_lab.cpp on the block's shapes (1 x MI355X, profiles/r3_gemm_pp.md): a
// workgroup needs ~1.6 / 1.4 / 1.2 us per K-step on the 256 / 192 / 128-token tile (the smaller tiles are bound by their loader phase,
// not by the matrix pipe) plus ~3 us per tile (8 with a GELU epilogue); the launch takes ceil(tiles / CUs) of those.  `steps`: K / 64
// for bf16, K / 128 for 8-bit operands — a K-step moves the same bytes and occupies the matrix pipe for the same cycles in both.
// Returns tj (tokens = 64 tj) and the tile count at that height.
static inline int pp_rounds_model(int M, int N, int steps, int mode, int* tiles_out) {
  static const float step_us[5] = {0.f, 0.f, 1.2f, 1.4f, 1.6f};
  const float tile_us = (mode == IFX_EPI_GELU_TANH ? 8.f : 3.f);
  int best = 0;
  float best_t = 1e30f;
  for (int tj = 4; tj >= 2; --tj) {
    const int tiles = ((M + 64 * tj - 1) / (64 * tj)) * ((N + 255) / 256);
    const float t = ((tiles + 255) / 256) * (steps * step_us[tj] + tile_us);      // rounds x time of one tile
    if (t < best_t) best_t = t, best = tj, *tiles_out = tiles;
  }
  return best;
}

// Which ping-pong tile (tokens = 64 tj) for a bf16 launch, 0 = none.  With K split in two (`split`: a gemm_pp_split shape and a
// workspace for it) there are twice the work items of half the length, 256- or 192-token tile only.
static inline int pick_pp(int M, int N, int K, int mode, bool split, bool small_split) {
  if (N % 64 != 0 || K % 64 != 0) return 0;
  // the split shapes at ANY row count (a row's summation order must not depend on it) unless the caller opted into the row-count
  // dependent in-workgroup splits for small launches
  if (split && gemm_pp_split(N, K) && ((M + 255) / 256) * ((N + 255) / 256) <= 1024 && !(small_split && M < 2048)) {
    // 256 or 192 tokens per tile: twice the work items of half the K-steps; the height that needs less time by the rounds model (the
    // bits do not depend on it).  4680 rows: 228 items = one round of the 256-token tile; 10800 rows (720p): 516 items = three rounds
    // against three shorter ones of the 192-token tile's 684
    const int tn = (N + 255) / 256, steps = K / 64 / 2;
    const int i4 = ((M + 255) / 256) * tn * 2, i3 = ((M + 191) / 192) * tn * 2;
    const float t4 = ((i4 + 255) / 256) * (steps * 1.6f + 9.f), t3 = ((i3 + 255) / 256) * (steps * 1.4f + 9.f);
    static const int allow3 = lab_env_int("IFX_PP_SPLIT_TJ3", 1);     // lab: 0 = the split on the 256-token tile only (rounds 3-4 before this rule)
    return (allow3 && i3 <= 2048 && t3 < t4 && mode != IFX_EPI_GELU_TANH) ? 3 : 4;
  }
  if (M < 1024) return 0;
  int tiles = 0;
  const int best = pp_rounds_model(M, N, K / 64, mode, &tiles);
  // 1024 .. 2047 rows (one MAGI chunk of a cp rank, 1519 rows): only where the chosen tile still gives most CUs a tile — 1519 x 8192 x
  // 3072 99 -> 70 us, x 12288 153 -> 128; with fewer tiles the LDS-DMA tiles with several workgroups per CU are ahead (1170 x 1536^2: 15 vs 27 us)
  return M < 2048 && tiles < 160 ? 0 : best;
}

// Split-K over two workgroups on the four-wave 256 x 256 tile (ifx_gemm_w4.hip): long-K launches whose 256 x 256 tiles fill less
// than half of the chip — the FFN down-projection, 4680 x 1536 x 8960: 114 tiles, 228 workgroups with the split.  Needs a caller
// workspace, so only ifx_gemm_bf16_ws takes this path.
// (measured on the FFN down-projection: 191 us against 164 us for the 128 x 128 two-per-CU tile — with 228 workgroups streaming
//  1 GB of operands the launch is paced by memory-side latency x bytes in flight, not by the K loop — so it is opt-in: variant 20)
static inline bool want_w4_splitk(int M, int N, int K) {
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  return K >= 4096 && (K / 64) % 2 == 0 && 2 * tiles <= 256 && 2 * tiles >= 160;
}

// LDS-DMA tile choice: score = (measured relative throughput of the tile at full occupancy) x (how well the launch's
// workgroups fill whole rounds of the chip).  256 CUs; the 64-wide tiles run two workgroups per CU.
static inline int pick_tile(int M, int N, int K, bool small_split) {
  struct Cand { int tile, bm, bn, slots; float base; };
  // 128x128 runs double-buffered with TWO workgroups per CU (64 KiB of LDS each): the co-resident workgroup hides the operand
  // latency better than the deep rings of the big tiles do — QKV 92 -> 83 us, O 38 -> 35, FFN down 150 -> 137 (tools/bench_gemm_tiles.py)
  // 256x192 (round 2): 7 % more outputs per round-microsecond than the two-per-CU 128x128 tile, 8 % fewer than 256x256; it wins
  // where 192-wide columns quantise better — the QKV projection, N = 4608 = 24 x 192: 456 tiles = 1.8 rounds against 1.3 of 256x256
  // (interleaved A/B, tools/scratch/ab_gemm_tiles.py: 4680x4608x1536 82.4 -> 75.3 us, 2340x4608x1536 47.1 -> 42.1, 2340x8960x1536
  // 83.7 -> 79.3; not picked, and slower, at 4680x8960 147 vs 142, 9360x4608 154 vs 144, 10800x4608 193 vs 181).  Same K order as the
  // other single-pass tiles: bit-identical outputs.
  static const Cand cands[] = {{kTile256x256, 256, 256, 256, 1.00f}, {kTile256x192, 256, 192, 256, 0.99f}, {kTile256x128, 256, 128, 256, 0.85f},
                               {kTile128x128, 128, 128, 512, 0.95f}, {kTile128x64, 128, 64, 512, 0.68f},   {kTile64x64, 64, 64, 512, 0.50f}};
  // Few output tiles (one rank's M = 4680 / P rows of a sequence-parallel shard): the parallelism has to come from K.  The Kg tiles
  // split K between wave groups of ONE workgroup (no workspace, fixed summation order).  Measured, tools/bench_gemm_tiles.py 585 / 2340:
  //   585x1536x1536 12.3 -> 9.8 us (kTile64x64Kg4), 585x1536x8960 43.2 -> 33.8 (kTile64x64Kg2)
  // They add the K halves / quarters in an order that is NOT the single-pass order, and whether a launch gets them depends on its ROW
  // count — so they are opt-in (ifx_set_option("gemm_small_split", 1); inferix_amd.sequence_parallel turns it on for its ranks, whose
  // row count is fixed by the rank count).  Without it the auto choice's summation order is a function of (N, K) alone: single pass
  // everywhere except the two-workgroup K split of ifx_gemm_pp.hip (gemm_pp_split(N, K), any row count, needs the workspace of
  // ifx_gemm_bf16_ws) — a row's bits do not change with the number of rows in the launch (tests/test_hip_kernels.py).
  const int kt = K / 64, wgs64 = ((M + 63) / 64) * ((N + 63) / 64);
  if (small_split) {
    if (wgs64 <= 256 && kt >= 64 && kt % 2 == 0) return kTile64x64Kg2;
    if (wgs64 <= 256 && kt >= 16 && kt % 4 == 0) return kTile64x64Kg4;
  }
  // one round of 128x64 workgroups at THREE per CU (two stages, 48 KiB) instead of 1.4 rounds at two per CU:
  //   585x8960x1536 31.8 -> 29.2 us, 585x4608x1536 19.2 -> 17.7, 1170x4608x1536 28.6 -> 27.2
  const int wgs12864 = ((M + 127) / 128) * ((N + 63) / 64);
  if (wgs12864 > 256 && wgs12864 <= 768) return kTile128x64s2;
  // (kTile128x128Kg2 on 128 < wgs128 <= 256 launches is worth 10 % on 2340x1536x8960; it stays opt-in because it would flip the umT5
  //  encoder's M = 512 x batch launches between summation orders.)
  // Long K and at least ~1.5 rounds of 256 x 256 tiles: the four-wave register-staged tile (ifx_gemm_w4.hip), whose K loop
  // needs a third less LDS bandwidth than the eight-wave tiles; its fixed cost per tile (one wave per SIMD: nothing overlaps the
  // prologue and the epilogue) is only amortised by K >= 2048.  MAGI-4.5B shapes, tools/bench_gemm_shapes.py: 6075 x 8192 x 3072
  // 326 -> 261 us, 6075 x 12288 x 3072 494 -> 409, 12150 x 3072 x 12288 1033 -> 900; the Wan block's K = 1536 GEMMs stay where they were.
  const int t256 = ((M + 255) / 256) * ((N + 255) / 256), rounds256 = (t256 + 255) / 256;
  if (K >= 2048 && t256 >= 384 && (float)t256 >= 0.7f * 256.f * rounds256) return kTileFourWave;
  int best = kTile64x64;
  float best_score = -1.f;
  for (const Cand& c : cands) {
    const int tm = (M + c.bm - 1) / c.bm, tn = (N + c.bn - 1) / c.bn, wgs = tm * tn;
    const int rounds = (wgs + c.slots - 1) / c.slots;
    const float edge = ((float)M * (float)N) / ((float)(tm * c.bm) * (float)(tn * c.bn));   // work in ragged edge tiles
    // less than one round of 256x256 tiles WITH a ragged edge: 128x128 wins (2340x4608: 46.6 vs 48.7 us, 1170x8960: 51.4 vs 53.9);
    // without one (the text encoder's 512x20480x4096) the big tile stays ahead (9.5 vs 10.0 ms per prompt)
    if (c.tile == kTile256x256 && wgs < c.slots && edge < 0.95f) continue;
    const float score = c.base * edge * (float)wgs / (float)(c.slots * rounds);
    if (score > best_score) best_score = score, best = c.tile;
  }
  return best;
}

// Under gemm_small_split (a sequence-parallel rank: row-count dependent summation orders are allowed) narrow-N launches whose 128 x 128
// tiles make ONE round of at most 256 workgroups take kTile128x128Kg2 — 128 x 128 with K split between the two wave groups of the
// workgroup — ahead of the ping-pong tiles: at 2340 rows (P = 2) 19 x 12 = 228 workgroups against 60-120 work items of the 256-token
// ping-pong tile.  tools/bench_gemm_tiles.py 2340: 1536^2 28.1 / 25.8 -> 23.3 / 19.3 us (+ residual / bias only), 1536 x 8960 102.6 -> 82.1.
static inline bool small_split_takes_tile12(int M, int N, int K, bool small_split) {
  const int wgs128 = ((M + 127) / 128) * ((N + 127) / 128);
  return small_split && N <= 2048 && (K / 64) % 2 == 0 && K >= 1024 && wgs128 > 128 && wgs128 <= 256;
}

// Shard-sized long-K launches (gemm_small_split): the 128-token ping-pong tile with K split over FOUR workgroups per tile where that
// makes one round of 129 .. 256 work items — a 4-way rank's FFN down-projection, 1170 x 1536 x 8960: 60 tiles x 4 = 240 items of 35
// K-steps, 52.0 us against 56.6 for the in-workgroup split 64 x 64 tiles (tools/bench_gemm_tiles.py 1170 0,27,28,29, round 5).  Measured
// and NOT taken everywhere else: 585 rows 46.7 (4-way) against 35.5, 2340 rows 80.2 (2-way) against 81.0, every K = 1536 launch behind
// the auto choice by 1.2 - 3x (the owner reads ks - 1 partial tiles: 128 KiB each through one CU).
static inline bool small_split_takes_pp_ks4(int M, int N, int K, bool small_split) {
  const int items = ((M + 127) / 128) * ((N + 255) / 256) * 4;
  return small_split && M < 2048 && N <= 2048 && N % 64 == 0 && K >= 4096 && K % 64 == 0 && (K / 64) % 4 == 0 && items > 128 && items <= 256;
}

// the plans --------------------------------------------------------------------------------------------------------------------------------
// ifx_gemm_bf16[_ws].  The order of the rules is the order a launch is claimed in.
static inline GemmPlan gemm_plan(const GemmRequest& r, int variant, bool small_split) {
  const GemmVariant v = gemm_variant_row(variant);
  const int M = r.M, N = r.N, K = r.K;
  const bool autov = v.kind == kGemmAuto;
  // without 16-byte epilogue vectors: the register-staged kernel, whatever gemm_variant asks for (it has no second destination)
  if (!r.wide_ok) return {r.y2 ? kGemmPathRefuseY2 : kGemmPathRegStaged};
  const long tiles128 = (long)((M + 127) / 128) * ((N + 255) / 256);
  auto pp = [&](int tj, int ks, size_t ws) { return GemmPlan{kGemmPathPp, -1, tj, ks, (int64_t)ws}; };
  // a K split happens only where the caller's workspace covers what it needs; on the 128-token ping-pong tile it also needs N and K in
  // multiples of 64 and gate groups of at least a wave's 64 token rows
  auto offered = [&](size_t need) { return need > 0 && r.ws_bytes >= (int64_t)need; };
  auto split128 = [&](size_t need) { return N % 64 == 0 && K % 64 == 0 && offered(need) && pp_epilogue_fits(r.mode, r.ops, 64); };
  const size_t w4 = gemm_w4_workspace_bytes(M, N, 2), stream_k = gemm_pp_stream_k_workspace_bytes(),
               parts = gemm_pp_small_workspace_bytes(M, N, autov ? 4 : v.ks), halves = gemm_pp_workspace_bytes(M, N, K);
  if (v.kind == kGemmW4SplitK && want_w4_splitk(M, N, K) && offered(w4)) return {kGemmPathW4, -1, 0, 2, (int64_t)w4};
  // stream-K on the 128-token ping-pong tile, meant for the shard-sized launches of a sequence-parallel rank (the K partition, hence the
  // summation order of a row, depends on the row count of the launch).
  // MEASURED AND NOT IN THE AUTO CHOICE (gemm_variant 26 only, profiles/r3_gemm_pp.md): at 585 rows a tile's K range is spread over 3-9
  // workgroups and the owner's epilogue reads that many partial sums one memory latency after the other — 36 us against 19 us (QKV), 79
  // against 37 us (FFN down) for the in-workgroup split tiles below.
  if (v.kind == kGemmPpStreamK && split128(stream_k) && tiles128 * (K / 64) >= 48) return pp(2, 0, stream_k);
  // second destination (ifx_epilogue.y2: the q|k|v projection storing its V columns straight into the KV cache): the ping-pong tiles
  // carry it; every other tile would drop the columns, so a launch that cannot take that path is an error, never a silent fallback
  if (r.y2) {
    if (!(r.mode == IFX_EPI_BIAS && N % 64 == 0 && r.ops.bias8 && (autov || v.kind == kGemmPp))) return {kGemmPathRefuseY2};
    const int tj = autov ? pick_pp(M, N, K, r.mode, false, small_split) : v.tj;
    return {kGemmPathPp, -1, tj ? tj : 2, 1, 0, true};
  }
  // the 128-token tile with K in 2 / 4 / 8 parts: the lab variants whatever the shape, auto where small_split_takes_pp_ks4 says
  if (v.kind == kGemmPpKParts && (K / 64) % v.ks == 0 && split128(parts) && tiles128 * (v.ks - 1) <= 1024) return pp(2, v.ks, parts);
  if (autov && small_split_takes_pp_ks4(M, N, K, small_split) && split128(parts)) return pp(2, 4, parts);
  if (autov && small_split_takes_tile12(M, N, K, small_split)) return {kGemmPathLdsDma, kTile128x128Kg2};
  // persistent ping-pong tiles: auto picks one for launches of at least 2048 rows (and for the split shapes at any row count); the gate
  // epilogue needs groups of at least a wave's token rows, the operands 16-byte rows.  A forced tile launches whatever the operands:
  // the launcher refuses what it cannot run.
  if (autov || v.kind == kGemmPp) {
    const bool split = v.takes_ws && offered(halves);
    const int tj = autov ? pick_pp(M, N, K, r.mode, split, small_split) : v.tj;
    // (the 256- and 192-token tiles are instantiated with the split: a caller that forces the 128-token tile on a split shape gets
    //  the unsplit launch, not an error; so does a forced 192-token tile whose tiling has more than 1024 tiles)
    const bool ks2 = split && tj >= 3 && (long)((M + 64 * tj - 1) / (64 * tj)) * ((N + 255) / 256) <= 1024;
    if (tj && (!autov || (N % 64 == 0 && pp_epilogue_fits(r.mode, r.ops, 32 * tj)))) return pp(tj, ks2 ? 2 : 1, ks2 ? halves : 0);
  }
  if (v.kind != kGemmRegStaged) return {kGemmPathLdsDma, v.tile >= 0 ? v.tile : pick_tile(M, N, K, small_split)};
  return {kGemmPathRegStaged};
}

// ifx_gemm_q8[_ws] / ifx_gemm_q8_quant_out, which read the same option: 1 / 2 = register-staged 128x128 / 64-byte-row LDS-DMA tiles,
// 3 = the LDS-DMA tiles, never the ping-pong tile, 22 .. 25 = the ping-pong tile of that height, anything else = by shape
static inline GemmPlan gemm_q8_plan(const GemmRequest& r, int variant, bool small_split) {
  const GemmVariant v = gemm_variant_row(variant);
  const int M = r.M, N = r.N, K = r.K;
  // FP8 / INT8 launches of >= 1024 rows (one MAGI chunk of a cp = 8 rank, 1519 rows: q 50 -> 33 us, proj 86 -> 55, fc2 148 -> 90,
  // tools/bench_q8.py), and the split shapes at any row count: the ping-pong tile
  if (r.wide_ok && variant != 1 && variant != 2 && variant != 3) {
    // K halves in two workgroups of the 256-token tile: the rule of the bf16 tiles on the K-STEP count (gemm_pp_split: N <= 2048, >= 64 steps
    // of 128 one-byte elements, an even number of them) — a function of N and K only, taken at ANY row count so that a row's summation
    // order does not depend on it (unless the caller opted into row-count dependent choices for shard-sized launches: gemm_small_split)
    const size_t need = N % 64 == 0 && K % 128 == 0 && !(small_split && M < 2048) ? gemm_pp_workspace_bytes(M, N, K / 2) : 0;
    const bool split = !r.qdiv && !(v.kind == kGemmPp && !v.takes_ws) && need > 0 && r.ws_bytes >= (int64_t)need &&
                       (r.mode != IFX_EPI_GATE_RES || r.ops.rows_per_group >= 128);
    int tiles = 0;
    int tj = v.kind == kGemmPp ? v.tj : (v.kind == kGemmAuto && split) ? 4
             : (M < 1024 || N % 64 != 0 || K % 128 != 0) ? 0 : pp_rounds_model(M, N, K / 128, r.mode, &tiles);
    if (r.mode == IFX_EPI_GATE_RES && r.ops.rows_per_group < 32 * tj) tj = r.ops.rows_per_group >= 64 ? 2 : 0;
    if (tj != 0 && N % 64 == 0 && r.qdiv16 && pp_epilogue_fits(r.mode, r.ops, 0))
      return {kGemmPathPp, -1, tj, split && tj == 4 ? 2 : 1, split && tj == 4 ? (int64_t)need : 0};
  }
  // large shapes: LDS-DMA tiles (256x256 with >= 2 rounds of tiles, else 256x128 when it fills the chip), 128-byte operand rows (two /
  // three stages) unless gemm_variant 2 asks for the 64-byte four-stage ring they replaced
  // (a 128x128 eight-wave tile at two workgroups per CU for the 1536- and 4608-wide outputs measured the same as 256x128)
  if (r.wide_ok && variant != 1) {
    auto wgs = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    if (wgs(256, 256) >= 512) return {kGemmPathLdsDma, variant != 2 ? kQ8Tile256x256 : kQ8Tile256x256Rows64};
    if (wgs(256, 128) >= 224) return {kGemmPathLdsDma, variant != 2 ? kQ8Tile256x128 : kQ8Tile256x128Rows64};
  }
  return {kGemmPathRegStaged};
}

}  // namespace ifx

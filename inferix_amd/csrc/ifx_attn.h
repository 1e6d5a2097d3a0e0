// Attention: what the entry points and launch plan (ifx_attn.hip) share with the multi-wave kernels and their launcher
// (ifx_attn_pp.hip) — two device helpers, the kernels' argument struct, the loop forms, THE table of schedules behind `attn_variant`,
// the launch request and the only prototypes of the functions that cross the two files.
#pragma once
#include "ifx_common.h"

// Compile-time knobs that size the LDS allocation or pick an instantiation, through the table below.  The launcher reads ITS OWN
// file's copy of the table (by AttnSchedule::variant), so a lab build that hands them to ifx_attn_pp.hip alone (tools/ablate_attn.sh)
// launches what it built; the plan only uses the rows' knob-independent fields (ng, qt, slots).
// PP_TRACE=1 (tools/trace_attn.sh): workgroup 0 stamps the cycle counter at the step boundaries of its first 64 tiles
// into the LSE buffer (as int64 [tile][wave][4]: M start, M end, V start, V end).  0 in the shipped library.
#ifndef PP_TRACE
#define PP_TRACE 0
#endif
#ifndef PP_PD
#define PP_PD 2        // DMA prefetch distance in tiles (issued from the softmax step); 3 measured slower
#endif
#ifndef PP_DUAL_FR
#define PP_DUAL_FR 6     // loop form of attn_variant 6 — 6: six-times unrolled over constant LDS slots; 3: the two-times unrolled form it replaced
#endif

namespace ifx {

namespace pp {
constexpr int KT = 64;
constexpr int HD = 128;
constexpr int PD = PP_PD;
constexpr int RK = PD + 1, RV = PD + 2;
constexpr int K_OFF = 0;
constexpr int LDS_BYTES = (RK + RV) * 16384;   // 114688
constexpr int LDS_SWP = 8 * 16384;              // software-pipelined schedule: 3 K tiles + 5 V tiles
constexpr int LDS_ALLOC = PP_TRACE ? LDS_SWP + 24576 : (LDS_BYTES > LDS_SWP ? LDS_BYTES : LDS_SWP);   // trace: 24 KiB of stamps behind the rings
constexpr int LDS_DUAL = 5 * 16384;             // 80 KiB: two four-wave workgroups per CU

// Loop forms: the values of FR in attn_fwd_pp_kernel<PAGED, SPLIT, NG, FR> (they are part of the kernel names that profiles show).
// Phase-locked wave groups (NG = 2 ping-pong, NG = 3 three-phase): the header of ifx_attn_pp.hip.
constexpr int FR_PLAIN = 0;
// Free-running (attn_variant 4): every wave runs QK(t) -> softmax(t) -> PV(t) for its own 32 queries with ONE
// workgroup barrier per tile and no phase assignment — the two waves of a SIMD drift apart by themselves, the older one takes
// the matrix pipe first and its softmax then overlaps with the younger wave's MFMAs (tools/probe_roles.hip).
constexpr int FR_FREE = 1;
// Software-pipelined (attn_variant 5): one wave keeps both pipes busy by itself, two times unrolled; reads K one tile ahead and V one
// tile behind (rings of 3 K + 5 V tiles).  Every form from here on is software-pipelined: FR >= FR_SWP.
constexpr int FR_SWP = 2;
// The software-pipelined loop in FOUR-wave workgroups of 128 queries, TWO of them per CU (80 KiB of
// LDS each: K ring 2, V ring 3).  The two waves of a SIMD then belong to different workgroups: no barrier couples them, so
// the older wave no longer waits ~600 cycles per tile for the younger one; the price is that each workgroup streams K/V itself.
// (PP_DUAL_FR = 3 only: not instantiated in the shipped library.)
constexpr int FR_SWP_DUAL = 3;
// attn_variant 7: the software-pipelined loop unrolled FOUR times over rings of 4 K + 4 V tiles, so that every LDS slot is
// a compile-time constant: a fragment read is `ds_read v_term offset:imm` with 12 lane terms computed once per kernel, where the
// two-times-unrolled loop re-derives its addresses every tile (56 of the 177 non-MFMA VALU instructions of a tile; the loop is
// bound by VALU issue).  V ring first (imm offsets reach 64 KiB), K ring behind it; K is requested three tiles ahead,
// V two (it is consumed two iterations later), which is what lets four V slots do.
constexpr int FR_U4 = 5;
// attn_variant 6: the same treatment for the two-per-CU form (rings of 2 K + 3 V tiles: unrolled six times).
constexpr int FR_U6_DUAL = 6;
// Exponent forms of the two above: the caller's scale * log2(e) is exactly 1 (q was scaled where it was produced): scores ARE exponents,
// and the softmax reference -m enters as the C operand of a score block's first MFMA, so exp2 is applied straight to the accumulator.
constexpr int FR_U4_PRE = 7;
constexpr int FR_U6_DUAL_PRE = 8;
// FR_U4 and FR_U4_PRE on v_mfma_f32_16x16x32_bf16 (option attn_mfma; the layout: header of ifx_attn_pp.hip): same schedule, rings,
// request stream and waits — the matrix instruction, the fragment lane maps, the S / P / O register layouts and the lane-group
// reductions differ.  Not rows of the table below: a launch of schedule 7 takes them when attn_plan says so (AttnForm).
constexpr int FR_U4_M16 = 9;
constexpr int FR_U4_PRE_M16 = 10;
}  // namespace pp

// single-instruction 3-input max (plain fmaxf on MFMA outputs makes hipcc emit a canonicalising v_max per input)
__device__ __forceinline__ float attn_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// max over the two half-waves that share a query column (lane, lane^32) without touching LDS:
// v_permlane32_swap exchanges vdst[32..63] with src[0..31] (verified by tools/probe_layouts).  Done in asm:
// the builtin called with two copies of one value is folded to a no-op by the optimiser.
__device__ __forceinline__ float attn_half_max(float x) {
  float a = x, b = x, r;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1\n\tv_max_f32 %2, %0, %1" : "+v"(a), "+v"(b), "=v"(r));
  return r;
}

// max over the four 16-lane groups that share a query column in the 16x16x32 forms: the half-wave exchange above, then
// v_permlane16_swap (rows 1, 3 of vdst <-> rows 0, 2 of src; verified by tools/probe_layouts), with the same wait states in front
__device__ __forceinline__ float attn_quad_max(float x) {
  const float h = attn_half_max(x);
  float a = h, b = h, r;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1\n\tv_max_f32 %2, %0, %1" : "+v"(a), "+v"(b), "=v"(r));
  return r;
}

struct AttnArgsPP {
  const unsigned short* q;
  unsigned short* out;      // nullptr: a partial launch — the fp32 partials stay in the workspace, nothing is merged
  float* lse;
  const unsigned short* k;
  const unsigned short* v;
  KvAddr ka;
  int q_rows, heads, kv_start, kv_len, num_slots, q_tiles, per_xcd, total;
  int ldq, ldo;             // elements between consecutive rows of q / out (heads * 128 unless the caller strides them)
  float scale, scale_log2;
  // split-KV (SPLIT kernels only): `splits` key chunks of `chunk_tiles` 64-key tiles each; chunk sp of (head, q tile)
  // writes a normalised fp32 partial O to part_o[sp][row][head][128] and its LSE to part_lse[sp][head][row]
  int splits, chunk_tiles;
  int kv_heads, q_per_kv;   // grouped-query attention: query head h reads kv head h / q_per_kv
  float* part_o;
  float* part_lse;
  // multi-range launch (n_ranges > 0, unsplit kernels only): query rows [rq0[r], rq1[r]) attend keys [rk0[r], rk1[r]); q tile ids
  // [rt0[r], rt0[r + 1]) of a head belong to range r (MAGI: the denoising chunks of one forward in ONE launch)
  int n_ranges;
  int rq0[8], rq1[8], rk0[8], rk1[8], rt0[9];
  // paged views (PAGED = 1 instantiations): key -> page by a multiply-high with `ps_magic` = floor(2^32 / page_size) + 1 (exact while
  // key * page_size < 2^32), on the SCALAR side, once per page (see the request lambda).  History: round 5 divided and loaded the table
  // entry per LANE in front of every K/V request (0.54x the contiguous kernel over 32760 keys), early round 6 read an LDS copy of the
  // table per lane (0.86x: the reads and their waits sit in the software-pipelined loop, the kernel was twice the contiguous one's size).
  unsigned ps_magic;
  // tests (option "attn_debug_counters"): a device word that counts the (wave, tile) pairs that took the rescale branch of the lazy
  // row maximum; nullptr in every normal launch (the increment sits inside the rare branch only)
  unsigned* dbg_rescales;
};

// One multi-wave schedule: what a launch needs to know about it.  THE list of schedules is the table below.
struct AttnSchedule {
  int variant;      // the attn_variant that names this row
  int ng;           // wave groups of four waves: workgroups of ng * 256 threads
  int fr, fr_pre;   // loop form, and the form launched instead when q carries scale * log2(e) already
  int qt;           // query rows per workgroup (128 * ng)
  int slots;        // workgroups the chip runs at once (256 CUs, one or two per CU): what the split heuristic fills
  int lds_bytes;    // dynamic LDS of a launch
  bool pipelined() const { return fr >= pp::FR_SWP; }
};
// attn_variant 2 .. 7 (1 is the four-wave kernel of ifx_attn.hip, 0 the automatic choice below)
constexpr AttnSchedule kAttnSchedules[6] = {
    /* 2 ping-pong, two phase-locked groups       */ {2, 2, pp::FR_PLAIN, pp::FR_PLAIN, 256, 256, pp::LDS_ALLOC},
    /* 3 three groups, 384-row tiles              */ {3, 3, pp::FR_PLAIN, pp::FR_PLAIN, 384, 256, pp::LDS_ALLOC},
    /* 4 free-running                             */ {4, 2, pp::FR_FREE, pp::FR_FREE, 256, 256, pp::LDS_ALLOC},
    /* 5 software-pipelined                       */ {5, 2, pp::FR_SWP, pp::FR_SWP, 256, 256, pp::LDS_ALLOC},
    /* 6 its four-wave form, two per CU           */ {6, 1, PP_DUAL_FR, PP_DUAL_FR == pp::FR_U6_DUAL ? pp::FR_U6_DUAL_PRE : PP_DUAL_FR, 128, 512, pp::LDS_DUAL},
    /* 7 unrolled four times over constant slots  */ {7, 2, pp::FR_U4, pp::FR_U4_PRE, 256, 256, pp::LDS_ALLOC},
};
inline const AttnSchedule& attn_schedule(int variant) { return kAttnSchedules[variant - 2]; }

// The schedule (2 .. 7) a launch of `q_rows` x `heads` takes under option value `variant`: 2 .. 7 name theirs; anything else gets 7,
// except that auto (0) takes 6 for launches whose rows fill 128-row tiles markedly better than 256-row tiles — one rank's 585 rows
// of an eight-way sequence-parallel shard: 5 x 128 (91 %) against 3 x 256 (76 %); one rank's clip 348 -> 332 ms
inline int attn_pick_variant(int variant, int q_rows, int heads) {
  if (variant >= 2 && variant <= 7) return variant;
  if (variant == 0 && q_rows > 0) {
    const int t256 = (q_rows + 255) / 256, t128 = (q_rows + 127) / 128;
    const float u256 = (float)q_rows / (256.f * t256), u128 = (float)q_rows / (128.f * t128);
    if (u128 > 1.1f * u256) return 6;
    // Launches of more than one round of workgroups: whole rounds are what costs.  256-row tiles run one per CU (256 slots), the
    // 128-row four-wave tiles two per CU (512 slots) at 0.953 of the rate (1061 vs 1113 TFLOP/s).  CausVid 720p: 10800
    // rows x 12 heads = 516 tiles = 2.02 rounds -> THREE rounds of 256-row tiles, but 1020 / 512 = 1.99 -> two of 128-row tiles
    // (measured 778 -> see profiles/r2_*); the 480p block (228 tiles, one round either way) stays on the 256-row schedule.
    if (heads > 0 && t256 * heads > 256) {
      const float c5 = (float)((t256 * heads + 255) / 256);
      const float c6 = (float)((t128 * heads + 511) / 512) / 0.953f;       // 1061 vs 1113 TFLOP/s at L = 32760 (both with constant LDS slots)
      if (c6 < 0.95f * c5) return 6;
    }
  }
  return 7;
}

// A request for the multi-wave kernels, as the entry points state it.
struct AttnLaunch {
  const unsigned short* q = nullptr;
  unsigned short* out = nullptr;
  float* lse = nullptr;
  const ifx_kv_view* kv = nullptr;
  int q_rows = 0, heads = 0;
  int ldq = 0, ldo = 0;                 // elements between rows of q / out; 0: heads * 128
  int kv_start = 0, kv_len = 0;         // keys [kv_start, kv_len); a range launch takes the hull of its key ranges instead
  float scale = 0.f;                    // <= 0: 1 / sqrt(128)
  int splits = 1;
  void* workspace = nullptr;
  // slot_cap == 0: self-contained launch (partials in slots [0, splits) of `workspace`, merged by the launcher when splits > 1).
  // slot_cap  > 0: PARTIAL launch for a workspace laid out for slot_cap slots: always writes fp32 partials, into slots
  //                [slot_base, slot_base + splits), no merge; *slots_used reports how many chunks were written.
  int slot_base = 0, slot_cap = 0, *slots_used = nullptr;
  // n_ranges > 0: query rows [q_ranges[2r], q_ranges[2r + 1]) attend keys [k_ranges[2r], k_ranges[2r + 1]), unsplit
  int n_ranges = 0;
  const int *q_ranges = nullptr, *k_ranges = nullptr;
};
// The loop form of a launch beyond its schedule: `pre` — q carries scale * log2(e) already, the exponent forms; `mfma16` — the
// 16x16x32 matrix instruction (schedule 7 only: FR_U4_M16 / FR_U4_PRE_M16).
struct AttnForm {
  bool pre = false, mfma16 = false;
};
// Whether a launch of `schedule` takes the 16x16x32 form under option value `mfma` (attn_mfma: 0 auto, 1 32x32x16, 2 16x16x32).  2 takes it
// wherever it is built: every launch of schedule 7.  Auto takes it for the launch classes where its median wall time beat the old
// form's minimum on random data (4680 rows x 12 heads, forms alternating in one process, profiles/r22_attn_mfma_shape.md): unsplit
// launches with prescaled q from 14040 keys on (-3.4 % .. -4.4 % up to 32760 keys, contiguous and paged).  The rule does not look at
// the view: a paged and a contiguous cache of the same keys give the same bits (tests/test_hip_full_size_properties.py), and over a
// contiguous cache 4680 and 9360 keys were within the run-to-run spread (+2 % / 0; the paged launches gained 4 % there too).
// Shorter launches, split and partial launches and unscaled q were not measured: they keep 32x32x16.
inline bool attn_pick_mfma16(int mfma, int schedule, bool pre, bool split, int nkeys) {
  if (schedule != 7 || mfma == 1) return false;
  if (mfma == 2) return true;
  return pre && !split && nkeys >= 14040;
}
// What a request comes to under option values `variant` and `mfma`: the kernels' arguments, the schedule (2 .. 7), the page kind
// (0 contiguous, 1 wave-uniform translation, 2 per lane) and the loop form.  Host arithmetic, no GPU call (ifx_attn.hip).
int attn_plan(const AttnLaunch& L, int variant, int mfma, AttnArgsPP& a, int& schedule, int& paged, AttnForm& form);
int launch_attn_pp(const AttnArgsPP& a, const AttnSchedule& s, int paged, bool write_partials, AttnForm form, dim3 grid,
                   hipStream_t stream);                                                             // ifx_attn_pp.hip
int launch_attn_merge(const float* workspace, int slot_cap, int slots_used, unsigned short* out, float* lse, int q_rows,
                      int heads, hipStream_t stream, int ldo = 0);                                  // ifx_attn_pp.hip
size_t attn_pp_workspace_bytes(int q_rows, int heads, int splits);
int attn_pp_split_heuristic(int q_rows, int heads, int nkeys, int qt, int slots);

}  // namespace ifx

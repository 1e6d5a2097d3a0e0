// Block-causal flash-attention forward, PING-PONG structure (gfx950, head_dim 128).
//
// Why: profiles of the 4-wave kernel (ifx_attn.hip) show MFMA utilisation 34-40 % although its loop is lean
// (32 MFMA + ~200 VALU + 48 LDS reads per 64-key tile per wave): per tile a wave needs ~1024 cycles of matrix
// pipe and ~1000 cycles of VALU issue, the two waves that share a SIMD belong to unrelated workgroups, and
// nothing makes one of them sit in its VALU part while the other owns the matrix pipe.
//
// Here the two waves of a SIMD are in the SAME 8-wave workgroup and alternate roles under workgroup barriers:
//
//   step M(t) : O^T += V(t-1)^T P(t-1)^T   then   S(t)^T = K(t) Q^T        32 MFMAs, 48 LDS fragment reads,
//                                                                           DMA issue of tile t+2 in the shadows
//   step V(t) : online softmax of S(t) -> P(t) (bf16), running max / sum, conditional in-place rescale of O
//
//   barrier index :   2t            2t+1          2t+2          2t+3
//   waves 0-3 (G0):   M(t)          V(t)          M(t+1)        V(t+1)
//   waves 4-7 (G1):   V(t-1)        M(t)          V(t)          M(t+1)
//
// so in every phase each SIMD has exactly one wave feeding the matrix pipe and one wave doing VALU work.
// K/V tiles (64 keys) arrive by LDS-DMA into rings (K: 3 slots, V: 4 slots, 16 KiB each = 112 KiB): tile t is
// issued two tiles ahead; one counted s_waitcnt vmcnt(4) per wave per tile retires exactly the tile that the
// next barrier publishes.  Layouts, swizzles, MFMA operand mapping and the k-slot relabelling that feeds P
// straight from the S accumulators are those of ifx_attn.hip.
//
// The four-times-unrolled constant-slot loop (attn_variant 7) exists in two matrix-instruction forms: v_mfma_f32_32x32x16_bf16 and
// v_mfma_f32_16x16x32_bf16 (FR_U4_M16 / FR_U4_PRE_M16, option attn_mfma).  The second form's fragment lane maps and its S / P / O
// register layouts stand at the head of its block in the kernel (`if constexpr (M16)`); tools/probe_layouts checks them.
#include <stdlib.h>
#include <type_traits>

#include "ifx_attn.h"
#include "ifx_attn_multi.h"
#include "ifx_launch.h"
#include "ifx_lds_dma.h"

// compile-time ablation for bottleneck studies (tools/ablate_attn.sh): 1 no DMA, 2 no softmax step,
// 4 no LDS fragment reads, 8 no MFMA.  0 in the shipped library.
#ifndef PP_ABLATE
#define PP_ABLATE 0
#endif
#ifndef PP_PACKED
#define PP_PACKED 1    // 1: v_pk_fma_f32 for the exponent arguments (measured +5 % over plain v_fma_f32), 0: plain
#endif
#ifndef PP_PRIO
#define PP_PRIO 2      // 1: raised priority around the MFMA step, 2: around the softmax step (measured best)
#endif
#ifndef PP_RING
#define PP_RING 6      // fragment-ring slots of the MFMA steps with two waves per SIMD (reads PP_RING - 1 batches ahead)
#endif
// software-pipelined schedule (FR_SWP and its unrolled forms) knobs
#ifndef PP_SWP_RING
#define PP_SWP_RING 4
#endif
#ifndef PP_SWP_BALANCE
#define PP_SWP_BALANCE 1
#endif
#ifndef PP_SWP_YIELD
#define PP_SWP_YIELD 0
#endif
#ifndef PP_SWP_PACKED
#define PP_SWP_PACKED 0
#endif
#ifndef PP_SWP_RECOMPUTE
#define PP_SWP_RECOMPUTE 1   // 1: lane-derived LDS address terms recomputed every tile; 0 keeps them live: 256 VGPRs + 170 B of spills, 1078 -> 783 TFLOP/s
#endif
#ifndef PP_MULTI
#define PP_MULTI 0     // 1: compiled as the body of ifx_attn_multi.hip — the kernel below becomes attn_fwd_multi_kernel(AttnMultiArgs), nothing else is emitted
#endif
#ifndef PP_GROUP
#define PP_GROUP 0     // 0: groups = waves 0-3 / 4-7 (waves w, w+4 share a SIMD); 1: even / odd waves
#endif

namespace ifx {

typedef float pp_f32x2 __attribute__((ext_vector_type(2)));
// (dma16, make_rsrc and why the DMA is issued from inline asm: ifx_lds_dma.h)

// wait until at most `tiles` DMA tile-groups (4 pieces each) of this wave are still in flight
__device__ __forceinline__ void pp_wait_tiles(int tiles) {
  if (tiles <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if (tiles == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if (tiles == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (tiles == 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
}

// NG = number of wave groups (4 waves each, one per SIMD): 2 = ping-pong (M | V), 3 = three-phase (M | V1 | V2).
// Why three: while one wave streams MFMAs, a SINGLE other wave on that SIMD gets a VALU instruction issued only every
// ~15 cycles, TWO other waves get one every ~8 (tools/probe_overlap.hip).  The softmax of a tile is ~110 VALU
// instructions against 32 MFMAs (1024 cycles): with one softmax wave per SIMD the step takes ~2000 cycles and the
// matrix pipe idles half the time (step trace, tools/trace_attn.sh); with two it fits in two MFMA steps.
// FR = loop form: the named values and what each is, in ifx_attn.h (pp::FR_*).
// PAGED = 1: the page (or segment) that holds key `kk` -> its key range [lo, hi) and the row offset physical - logical.  All scalar;
// the table entry comes through the scalar cache (s_load_dword from inline asm with its own wait: a compiler-visible load would
// put lgkmcnt / vmcnt waits for it into the software-pipelined loop around the call).
__device__ __forceinline__ void pp_page_range(const KvAddr& ka, unsigned ps_magic, int kk, int& lo, int& hi, int& off) {
  if (ka.pt == nullptr) {
    const bool up = ka.seg_split > 0 && kk >= ka.seg_split;
    lo = up ? ka.seg_split : 0;
    hi = (up || ka.seg_split <= 0) ? 0x7fffffff : ka.seg_split;
    off = up ? ka.seg_delta : 0;
    return;
  }
  const int pg = (int)__umulhi((unsigned)kk, ps_magic);
  int entry;
  asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(entry) : "s"(ka.pt), "s"(pg * 4) : "memory");
  lo = pg * ka.ps;
  hi = lo + ka.ps;
  off = entry * ka.ps - lo;
}

// PAGED: 0 = contiguous cache (logical row = physical row); 1 = page table with pages of at least 3 rows, or a two-segment view —
// wave-uniform translation (a 4-key request piece spans at most two pages); 2 = one- and two-row pages, tables whose multiply-high
// page index would not be exact — per-lane translation (KvAddr::slot: a division and a table load per request), instantiated for the
// plain two-group schedule only (the launcher routes such views there).
#if PP_MULTI
// Several unsplit launches in one (ifx_attn_fwd_multi): workgroup `blockIdx.x` is tile blockIdx.x / heads of the launch's tile table
// (items in the plan's order, longest key range first; tile-major like the range launch) for head blockIdx.x % heads.  This prologue
// resolves the tile's item into `A`, the arguments of that item's own single launch — pointers, strides, key range, capacity, page
// map — with scalar selects over the by-value table; everything behind it is the kernel as the single launch runs it.
template <int PAGED, bool SPLIT, int NG, int FR = 0>
__global__ __launch_bounds__(NG * 256, NG == 1 ? 2 : 1) void attn_fwd_multi_kernel(AttnMultiArgs M) {
  static_assert(!SPLIT && PAGED <= 1, "the multi launch is unsplit, over contiguous or wave-uniform paged views");
  if ((int)blockIdx.x >= M.total) return;
  const int m_gqt = (int)blockIdx.x / M.heads, m_head = (int)blockIdx.x - m_gqt * M.heads;
  AttnItemArgs it = M.item[0];
  int m_t0 = 0;
#pragma unroll
  for (int i = 1; i < kAttnMultiItems; ++i)
    if (i < M.n_items && m_gqt >= M.rt0[i]) it = M.item[i], m_t0 = M.rt0[i];
  const int m_qt = m_gqt - m_t0;
  AttnArgsPP A = {};
  A.q = it.q, A.out = it.out, A.k = it.k, A.v = it.v;
  A.ka = KvAddr{it.pt, it.ps, 0, 0};
  A.q_rows = it.q_rows, A.heads = M.heads, A.kv_start = it.kv_start, A.kv_len = it.kv_len, A.num_slots = it.num_slots;
  A.ldq = it.ldq, A.ldo = it.ldo;
  A.scale = M.scale, A.scale_log2 = M.scale_log2;
  A.splits = 1;
  A.kv_heads = M.kv_heads, A.q_per_kv = M.q_per_kv;
  A.ps_magic = it.ps_magic;
  A.dbg_rescales = M.dbg_rescales;
#else
template <int PAGED, bool SPLIT, int NG, int FR = 0>
__global__ __launch_bounds__(NG * 256, NG == 1 ? 2 : 1) void attn_fwd_pp_kernel(AttnArgsPP A) {
#endif
  using namespace pp;
  constexpr int QT = 128 * NG;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool M16 = FR == FR_U4_M16 || FR == FR_U4_PRE_M16;            // the 16x16x32 form of FR_U4 / FR_U4_PRE
  constexpr bool SWP = FR >= FR_SWP, DUAL = FR == FR_SWP_DUAL || FR == FR_U6_DUAL || FR == FR_U6_DUAL_PRE, U4 = FR == FR_U4 || FR == FR_U4_PRE || M16,
                 U6 = FR == FR_U6_DUAL || FR == FR_U6_DUAL_PRE, CS = U4 || U6;   // CS: constant LDS slots
  constexpr bool PRE = FR == FR_U4_PRE || FR == FR_U6_DUAL_PRE || FR == FR_U4_PRE_M16;   // scores are exponents
  // DMA prefetch distance and LDS rings of this schedule (FR_SWP reads K one tile ahead and V one tile behind)
  constexpr int PD = (FR == FR_SWP || U4) ? 3 : pp::PD, RK = DUAL ? 2 : (U4 ? 4 : (FR == FR_SWP ? 3 : pp::RK)),
                RV = DUAL ? 3 : (U4 ? 4 : (FR == FR_SWP ? 5 : pp::RV));
  constexpr int K_OFF = CS ? RV * 16384 : 0, V_OFF = CS ? 0 : RK * 16384;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = (NG == 2 && PP_GROUP) ? (wave & 1) : (wave >> 2);
  const bool loader = wave < 8;          // 32 DMA pieces per tile = 8 waves x 4 (a third group only computes)
  const int hi = lane >> 5, l31 = lane & 31;

  const int xcd = blockIdx.x & 7, slot_i = blockIdx.x >> 3;
  // Multi-range launches hand tiles of DIFFERENT cost (key ranges of 2 .. 5 chunks) out in launch order, most expensive first: the
  // contiguous per-XCD blocks of the uniform case would give one XCD all the long tiles (measured: 780 -> 477 TFLOP/s on the MAGI
  // rank shape), and with grouped-query heads sharing one K/V stream there is no per-head L2 locality to protect.
#if PP_MULTI
  const int wi = (int)blockIdx.x;
  const int head = m_head, qt = m_qt, sp = 0;      // (xcd / slot_i unused: tiles go out in launch order, as in a range launch)
  (void)xcd, (void)slot_i;
#else
  const int wi = (!SPLIT && A.n_ranges > 0) ? (int)blockIdx.x : xcd * A.per_xcd + slot_i;
  if ((A.n_ranges == 0 && slot_i >= A.per_xcd) || wi >= A.total) return;
  // work order (head, key chunk, q tile): the q tiles that stream the same K/V chunk sit on one XCD's L2
  int head, qt, sp = 0;
  if (SPLIT) {
    const int per_head = A.splits * A.q_tiles;
    head = wi / per_head;
    const int rem = wi - head * per_head;
    sp = rem / A.q_tiles;
    qt = rem - sp * A.q_tiles;
  } else if (A.n_ranges > 0) {
    qt = wi / A.heads;                     // tile-major: the longest range's tiles of every head first
    head = wi - qt * A.heads;
  } else {
    head = wi / A.q_tiles;
    qt = wi - head * A.q_tiles;
  }
#endif
  int kv_s = SPLIT ? A.kv_start + sp * A.chunk_tiles * KT : A.kv_start;
  int kv_e = SPLIT ? min(A.kv_len, kv_s + A.chunk_tiles * KT) : A.kv_len;
  int q_base = qt * QT, q_lim = A.q_rows;
  if (!SPLIT && A.n_ranges > 0) {
    int r = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
      if (i < A.n_ranges && qt >= A.rt0[i]) r = i;
    q_base = A.rq0[r] + (qt - A.rt0[r]) * QT;
    q_lim = A.rq1[r];
    kv_s = A.rk0[r];
    kv_e = A.rk1[r];
  }
  const int row_stride = A.heads * HD;

  const int qrow = q_base + wave * 32 + l31;
  const int qrow_c = min(qrow, q_lim - 1);
  bf16x8 qf[8];
  if constexpr (M16) {      // B fragments of 32 d x 16 queries: qf[4 qb + step] = query 16 qb + lane % 16, d 32 step + 8 (lane / 16) ..
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int qr = min(q_base + wave * 32 + 16 * qb + (lane & 15), q_lim - 1);
      const unsigned short* qp = A.q + (size_t)qr * A.ldq + head * HD + (lane >> 4) * 8;
#pragma unroll
      for (int st = 0; st < 4; ++st) qf[4 * qb + st] = *reinterpret_cast<const bf16x8*>(qp + st * 32);
    }
  } else {
    const unsigned short* qp = A.q + (size_t)qrow_c * A.ldq + head * HD + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
  }
  // Retire the Q loads HERE with a wait the compiler can see (vmcnt(0), expcnt/lgkmcnt untouched).  Otherwise it
  // carries them as "maybe pending" around the loop back-edge and protects every first use of qf in the loop with
  // vmcnt(7..0) — which, since the asm-issued DMA below shares the counter, drains the K/V prefetch queue every tile.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  // ---- LDS-DMA through buffer descriptors (buffer_load_dwordx4 ... lds): a tile is 16 K pieces + 16 V pieces of
  //      1 KiB (4 key rows x 256 B); wave w moves pieces w and w+8.  Per lane only a 32-bit voffset per piece is
  //      live (row * row_bytes + swizzled source chunk); the tile offset is a scalar soffset.  Rows beyond the
  //      descriptor's range (keys >= kv_len in the ragged last tile) read as ZERO by the hardware bounds check.
  const int row_bytes = A.kv_heads * HD * 2;     // cache row pitch
  const int kvh = head / A.q_per_kv;
  // piece r = 1 is 32 key rows below piece 0 (same swizzle phase): one voffset per matrix, +32 rows on the scalar side
  const int nkeys = kv_e - kv_s;
  const int NT = (nkeys + KT - 1) / KT;
  // identity page map: descriptor covers logical tokens [0, kv_len); paged: whole cache, keys clamped by hand
  const unsigned valid_rows = PAGED ? (unsigned)A.num_slots : (unsigned)kv_e;
  const unsigned nrec = (valid_rows - 1) * (unsigned)row_bytes + 256u;
  const v4i krs = make_rsrc(A.k + kvh * HD, nrec);
  const v4i vrs = make_rsrc(A.v + kvh * HD, nrec);
  const unsigned lds00 = (unsigned)(unsigned long long)(lds_ptr_t)smem;
  const int last_key = kv_e - 1;
  int pc_lo = 0, pc_hi = 0, pc_off = 0;              // PAGED = 1: key range and (physical - logical) row offset of the page of the last request
  // The two lane offsets of a request (K and V rows of this wave's pieces: row * row_bytes + swizzled 16-byte chunk) in ONE register kept
  // across the loop: row_bytes is a multiple of 256, so bits 0-7 hold the K chunk, bits 8-27 the row term and bits 28-31 the V chunk index.
  // A call unpacks its offset with one (K) or three (V) VALU instructions instead of re-deriving it from the lane id with seven or eight —
  // the older wave of every SIMD issues eight requests per tile and the loop is bound by instruction issue.  Pieces of wave `wv` != wave
  // (wave + 4: sixteen rows on) have the same swizzle phase: the same lane offsets.
  int lane_pack;
  {
    const int ln0 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int pc0 = ln0 & 15, row0 = wave * 4 + (ln0 >> 4);          // the row term holds the lane's row INSIDE the piece (0 .. 3) only:
    lane_pack = (ln0 >> 4) * row_bytes + ((pc0 ^ (row0 & 15)) << 4) +   // the piece's first row is the scalar side's business
                (int)((unsigned)((((pc0 >> 2) ^ (row0 & 3)) << 2) | (pc0 & 3)) << 28);
  }
  auto issue_w = [&](int t, int wv, int what = 3) {  // the pieces that belong to wave `wv` (rows 4 wv .. 4 wv + 3 of each half); what: 1 K, 2 V
    // (opaque: hipcc otherwise precomputes every (ring slot, half, wave) destination address of the unrolled loop — 32 loop-invariant
    //  scalars, spilled to lanes and fetched with a v_readlane in front of each request; one s_add per request is cheaper in a loop
    //  that is bound by VALU issue)
    unsigned lds0 = lds00 + wv * 1024;
    asm volatile("" : "+s"(lds0));
    int ln = 0;                                     // lane id: only the boundary / per-lane paths of the paged forms use it
    if constexpr (PAGED != 0) {
      ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      asm volatile("" : "+v"(ln));                  // recomputed, not kept live (see stepM)
    }
    int lp = lane_pack;
    asm volatile("" : "+v"(lp));                    // (unpacked at every call: two derived registers kept live would spill)
    const int k_lane = lp & 0x0fffffff;
    const int v_lane = (lp & 0x0fffff00) | (int)(((unsigned)lp >> 28) << 4);
    const unsigned kb = lds0 + K_OFF + (t % RK) * 16384;
    const unsigned vb = lds0 + V_OFF + (t % RV) * 16384;
    if (!PAGED) {
      int rb = row_bytes;
      asm volatile("" : "+s"(rb));                  // (opaque for the same reason: one s_mul per request instead of 16 spilled row offsets)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int soff = (kv_s + t * KT + wv * 4 + 32 * r) * rb;     // first row of the piece
        if (what & 1) dma16(krs, kb + r * 8192, k_lane, soff);
        if (what & 2) dma16(vrs, vb + r * 8192, v_lane, soff);
      }
    } else if constexpr (PAGED == 1) {
      // A piece is four CONSECUTIVE keys, nearly always inside ONE page: the translation is wave-uniform.  The physical row of
      // the piece's first key goes into the scalar offset, the lane offsets are the contiguous cache's; the page of the last request is
      // remembered in three scalars (a page is ~24 tiles) and looked up again — one scalar load from the table, inline asm so that the
      // compiler's wait counters never see it — only when a request leaves it.  The common path has no memory operation and two VALU
      // instructions per request.  Keys behind the last one read the last key's row (as the per-lane form did: finite values under
      // the mask) by a lane-row clamp, and a piece that straddles a page boundary adds the next page's offset to its upper lanes:
      // both in one scalar branch that only boundary pieces take.
      const int key00 = __builtin_amdgcn_readfirstlane(kv_s + t * KT + wv * 4);
      if (key00 >= pc_lo && key00 + 35 < pc_hi && key00 + 35 <= last_key) {
        // both pieces of the wave (keys key00 .. +3 and key00 + 32 .. +35) inside the remembered page and the key range: the
        // contiguous kernel's requests with another scalar offset (the loop is bound by instruction issue: every scalar
        // instruction per request shows)
        const int soff = (key00 + pc_off) * row_bytes;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (what & 1) dma16(krs, kb + r * 8192, k_lane, soff + r * 32 * row_bytes);
          if (what & 2) dma16(vrs, vb + r * 8192, v_lane, soff + r * 32 * row_bytes);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int key0 = key00 + 32 * r;
          const int kk = min(key0, last_key);
          if (kk < pc_lo || kk >= pc_hi) pp_page_range(A.ka, A.ps_magic, kk, pc_lo, pc_hi, pc_off);
          int soff = (kk + pc_off) * row_bytes;
          int adj = 0;
          if (kk + 3 > last_key || kk + 3 >= pc_hi) {        // rare: the ragged last piece of the key range, or a piece that runs into the next page
            const int j = min(ln >> 4, last_key - kk);
            adj += ((ln >> 4) - j) * row_bytes;
            if (kk + min(3, last_key - kk) >= pc_hi) {      // its rows from pc_hi on live in the NEXT page (a piece spans at most two: page_size >= 3)
              int lo2, hi2, off2;
              pp_page_range(A.ka, A.ps_magic, pc_hi, lo2, hi2, off2);
              // whole physical row per lane (the next page may lie anywhere, and a lane offset cannot go negative); scalar offset 0
              adj -= (kk + ((kk + j >= pc_hi) ? off2 : pc_off)) * row_bytes;
              soff = 0;
            }
          }
          if (what & 1) dma16(krs, kb + r * 8192, k_lane - adj, soff);
          if (what & 2) dma16(vrs, vb + r * 8192, v_lane - adj, soff);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int key = min(kv_s + t * KT + wv * 4 + (ln >> 4) + 32 * r, last_key);
        const int delta = (A.ka.slot(key) - (ln >> 4)) * row_bytes;     // physical row instead of the row inside the piece
        if (what & 1) dma16(krs, kb + r * 8192, k_lane + delta, 0);
        if (what & 2) dma16(vrs, vb + r * 8192, v_lane + delta, 0);
      }
    }
  };
  auto issue = [&](int t) { issue_w(t, wave); };

  if constexpr (M16) {
    // ================= FR_U4 / FR_U4_PRE on v_mfma_f32_16x16x32_bf16 (option attn_mfma) ===========================================
    // Same schedule as the 32x32x16 form below (PV(t-1) || QK(t+1) || softmax(t), rings of 4 K + 4 V tiles in constant slots, the
    // request stream, the counted waits, one barrier per tile, the lazy maximum with its redo path, -m as the C operand).  Layout
    // (g = lane / 16, i = lane % 16; checked by tools/probe_layouts):
    //   S^T block (kb, qb) = 16 keys x 16 queries, f32x4: lane holds query 16 qb + i, keys 16 kb + 4 g + 0..3.
    //     A = K fragment (kb, step): key 16 kb + i, d 32 step + 8 g .. + 7 — one ds_read_b128, conflict-free under the K image's XOR
    //     with the row; it feeds the two query blocks.  B = qf[4 qb + step].
    //   P^T operand (ks, qb) of the 32-key step ks: the lane's S values of key blocks 2 ks and 2 ks + 1, packed in place: k-slots
    //     8 g + 0..3 = keys 32 ks + 4 g + 0..3, k-slots 8 g + 4..7 = keys 32 ks + 16 + 4 g + 0..3 (no cross-lane move).
    //   V^T fragment (ks, db) = 16 d x 32 keys with that key-to-slot map: two ds_read_b64_tr_b16 of keys 32 ks + 4 g .. + 3 and
    //     + 16, d 16 db .. + 15 (2-way bank conflict: the two groups of a half read rows 4 apart of one 32-byte column).
    //   O^T block (db, qb), f32x4: query 16 qb + i, d 16 db + 4 g + 0..3.
    //   A lane owns two queries x 16 scores of a tile; row sums stay lane-partial, maxima and final sums reduce over the four groups.
    const int g16 = lane >> 4, i16 = lane & 15;
    f32x4 o[8][2];
#pragma unroll
    for (int db = 0; db < 8; ++db) o[db][0] = o[db][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.f, 0.f};
    const float c2 = PRE ? 1.0f : A.scale_log2;
    f32x4 sA[4][2], sB[4][2];
    bf16x8 pA[2][2], pB[2][2];
    pA[0][0] = pA[0][1] = pA[1][0] = pA[1][1] = bf16x8{};
    pB[0][0] = pB[0][1] = pB[1][0] = pB[1][1] = bf16x8{};          // P(-1) = 0
    f32x4 negm[2];                                                  // PRE: -m of the lane's two queries (MFMA C operands)
    auto set_negm = [&](int qb, float m) {
      negm[qb] = f32x4{-m, -m, -m, -m};
      asm volatile("" : "+v"(negm[qb]));
    };
    if (PRE) {
      set_negm(0, 0.f);
      set_negm(1, 0.f);
    }
    int kterm[4], vterm[4];      // lane terms of the fragment reads, once per kernel (K_OFF folded into the K terms; V_OFF = 0)
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      kterm[st] = K_OFF + i16 * 256 + (((4 * st + g16) ^ i16) << 4);
      asm volatile("" : "+v"(kterm[st]));
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      vterm[c] = (4 * g16 + (i16 >> 2)) * 256 + ((c ^ (i16 >> 2)) << 6) + ((i16 & 3) << 3);
      asm volatile("" : "+v"(vterm[c]));
    }
    auto mfma16 = [](const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); };
    auto ld_v = [&](int vbase, int ks, int db) -> bf16x8 {      // vbase: byte offset of the V tile
      const unsigned char* a0 = smem + vterm[db >> 1] + (vbase + 32 * ks * 256 + (db & 1) * 32);
      const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
      const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0 + 4096));
      return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    auto ld_k = [&](int kbase, int kb, int st) -> bf16x8 {      // kbase: byte offset of the K tile inside the K ring
      return *reinterpret_cast<const bf16x8*>(smem + kterm[st] + (kbase + 16 * kb * 256));
    };
    auto mask_ragged = [&](int t, f32x4(&sx)[4][2]) {
      int kidx = t * KT + 4 * g16;                     // (opaque: see the 32x32x16 form)
      asm volatile("" : "+v"(kidx));
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kidx + 16 * kb + r >= nkeys) sx[kb][qb][r] = -INFINITY;
    };
    auto true_max = [&](f32x4(&sx)[4][2], int qb, float floor_v) -> float {
      float mx = attn_max3(__builtin_fmaxf(sx[0][qb][0], sx[1][qb][0]), floor_v, floor_v);
#pragma unroll
      for (int r = 1; r < 4; ++r) mx = attn_max3(mx, sx[0][qb][r], sx[1][qb][r]);
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = attn_max3(mx, sx[2][qb][r], sx[3][qb][r]);
      return attn_quad_max(mx);
    };
    auto exp_plain = [&](f32x4(&sx)[4][2], bf16x8(&px)[2][2], int qb, float mc) -> float {      // non-interleaved (redo path)
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const float p0 = __builtin_amdgcn_exp2f(sx[kb][qb][r] * c2 - mc);
          const float p1 = __builtin_amdgcn_exp2f(sx[kb][qb][r + 1] * c2 - mc);
          a0 += p0;
          a1 += p1;
          px[kb >> 1][qb][4 * (kb & 1) + r] = static_cast<__bf16>(p0);
          px[kb >> 1][qb][4 * (kb & 1) + r + 1] = static_cast<__bf16>(p1);
        }
      return a0 + a1;
    };
    // (plain multiplies, unconditional inside the rare branch: with the 32x32x16 form's per-element inline asm under a second branch the
    //  allocator split the O tuples and spilled lane terms and Q fragments in the hot path — 412 B of scratch, reloads that drain the
    //  request queue through the shared vmcnt)
    auto rescale_o = [&](int qb, float alpha) {
#pragma unroll
      for (int db = 0; db < 8; ++db) o[db][qb] *= alpha;
    };
    // iteration t: sC = S(t) -> pC = P(t) (softmax), pP = P(t-1) -> O (PV), sN = S(t+1) (QK).  16 batches of two fragments and four
    // MFMAs (each fragment feeds both query blocks), one pair of exponentials per batch:
    //   PV batch j = (key step ks = j >> 2, d blocks 2 (j & 3), 2 (j & 3) + 1)        j = 0..7
    //   QK batch q = (key block kb = q >> 1, d steps 2 (q & 1), 2 (q & 1) + 1)        q = j - 8 = 0..7
    //   softmax piece j = (ks = j >> 3, qb = (j >> 2) & 1, word w = j & 3 of the P operand): registers 2 (w & 1), + 1 of S block 2 ks + (w >> 1)
    auto body = [&](f32x4(&sC)[4][2], f32x4(&sN)[4][2], bf16x8(&pC)[2][2], bf16x8(&pP)[2][2], auto kslot_c, auto vslot_c, float(&tsum)[2]) {
      constexpr int KSLOT = decltype(kslot_c)::value, VSLOT = decltype(vslot_c)::value;
      constexpr int RDs = PRE ? 2 : PP_SWP_RING, LAs = RDs - 1;
      bf16x8 fs[RDs][2];
      auto load = [&](int j) {
        bf16x8(&f)[2] = fs[j % RDs];
        if (j < 8) {
#pragma unroll
          for (int e = 0; e < 2; ++e) f[e] = ld_v(VSLOT * 16384, j >> 2, 2 * (j & 3) + e);
        } else {
          const int q = j - 8;
#pragma unroll
          for (int e = 0; e < 2; ++e) f[e] = ld_k(KSLOT * 16384, q >> 1, 2 * (q & 1) + e);
        }
      };
      auto mma1 = [&](int j, int e, int qb) {
        const bf16x8& f = fs[j % RDs][e];
        if (j < 8) {
          const int ks = j >> 2, db = 2 * (j & 3) + e;
          o[db][qb] = mfma16(f, pP[ks][qb], o[db][qb]);
        } else {
          const int q = j - 8, kb = q >> 1, st = 2 * (q & 1) + e;
          if (st == 0) sN[kb][qb] = mfma16(f, qf[4 * qb + st], PRE ? negm[qb] : f32x4{0.f, 0.f, 0.f, 0.f});     // PRE: S - m
          else sN[kb][qb] = mfma16(f, qf[4 * qb + st], sN[kb][qb]);
        }
      };
      float p0 = 0.f, p1 = 0.f, e1 = 0.f;
      float acc4[4] = {0.f, 0.f, 0.f, 0.f};             // two row-sum chains per query block
      u32x4 pw[2][2];                                    // P(t) as packed bf16 pairs
      const float mc[2] = {m_run[0] * c2, m_run[1] * c2};
#pragma unroll
      for (int j = 0; j < LAs; ++j) load(j);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int ks = j >> 3, qb = (j >> 2) & 1, w = j & 3, kb = 2 * ks + (w >> 1), r0 = 2 * (w & 1);
        __builtin_amdgcn_sched_barrier(0);
        if (j + LAs < 16) load(j + LAs);
        mma1(j, 0, 0);
        if (PRE) {                                     // the score is the exponent
          p0 = __builtin_amdgcn_exp2f(sC[kb][qb][r0]);
          e1 = sC[kb][qb][r0 + 1];
        } else {
          p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sC[kb][qb][r0], c2, -mc[qb]));
          e1 = __builtin_fmaf(sC[kb][qb][r0 + 1], c2, -mc[qb]);
          asm volatile("" : "+v"(e1));
        }
        mma1(j, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma1(j, 1, 0);
        p1 = __builtin_amdgcn_exp2f(e1);
        mma1(j, 1, 1);
        // (one wait state between v_exp_f32 and a VALU read of its result: the hazard recogniser does not look into inline asm)
        asm volatile("s_nop 0\n\tv_add_f32 %0, %0, %1" : "+v"(acc4[2 * qb]) : "v"(p0));
        asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc4[2 * qb + 1]) : "v"(p1));
        unsigned pk;
        asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(p0), "v"(p1));
        pw[ks][qb][w] = pk;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) pC[ks][qb] = __builtin_bit_cast(bf16x8, pw[ks][qb]);
      tsum[0] = acc4[0] + acc4[1];
      tsum[1] = acc4[2] + acc4[3];
    };
    auto iteration = [&](int t, f32x4(&sC)[4][2], f32x4(&sN)[4][2], bf16x8(&pC)[2][2], bf16x8(&pP)[2][2], auto kslot_c, auto vslot_c) {
      // own pieces of tile t+1 landed (t+2 may stay in flight); only waves 0-3 have any (8 per tile)
      if (t + 2 < NT) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                    // tile t+1 complete for everyone; K(t) and V(t-2) are free
      if (wave < 4) {                                  // K three tiles ahead, V two: four slots each
        if (t + 3 < NT) {
          issue_w(t + 3, wave, 1);
          issue_w(t + 3, wave + 4, 1);
        }
        if (t + 2 < NT) {
          issue_w(t + 2, wave, 2);
          issue_w(t + 2, wave + 4, 2);
        }
      }
      if (t == NT - 1 && (nkeys & (KT - 1))) mask_ragged(t, sC);
      float tsum[2];
      body(sC, sN, pC, pP, kslot_c, vslot_c, tsum);
      if (__any(!(tsum[0] < 1048576.f) || !(tsum[1] < 1048576.f))) {      // rare: this tile outgrew the reference (inf / NaN land here too)
        if (A.dbg_rescales != nullptr && lane == 0) atomicAdd(A.dbg_rescales, 1u);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          if (PRE) {                                   // sC holds S(t) - m_run, sN already holds S(t+1) - m_run
            const float d = true_max(sC, qb, 0.f);     // >= 0: how far this tile's maximum lies above the reference
            const float alpha = __builtin_amdgcn_exp2f(-d);
            tsum[qb] = exp_plain(sC, pC, qb, d);
            m_run[qb] += d;
            l_run[qb] *= alpha;
            rescale_o(qb, alpha);
            set_negm(qb, m_run[qb]);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
              for (int r = 0; r < 4; ++r) sN[kb][qb][r] -= d;
          } else {
            const float m_new = true_max(sC, qb, m_run[qb]);
            const float alpha = __builtin_amdgcn_exp2f((m_run[qb] - m_new) * c2);
            m_run[qb] = m_new;
            tsum[qb] = exp_plain(sC, pC, qb, m_new * c2);
            l_run[qb] *= alpha;
            rescale_o(qb, alpha);
          }
        }
      }
      l_run[0] += tsum[0];
      l_run[1] += tsum[1];
    };
    // ---- prologue: V slot 3 is read (times P(-1) = 0) by the PV of iteration 0 before anything was copied there
    *reinterpret_cast<u32x4*>(smem + V_OFF + 3 * 16384 + tid * 32) = u32x4{0, 0, 0, 0};
    *reinterpret_cast<u32x4*>(smem + V_OFF + 3 * 16384 + tid * 32 + 16) = u32x4{0, 0, 0, 0};
    if (wave < 4) {                                    // K(0), V(0), K(1), V(1), K(2): everything but K(2) has to land now
      issue_w(0, wave, 3);
      issue_w(0, wave + 4, 3);
      if (NT > 1) {
        issue_w(1, wave, 3);
        issue_w(1, wave + 4, 3);
      }
      if (NT > 2) {
        issue_w(2, wave, 1);
        issue_w(2, wave + 4, 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)                     // S(0)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        sA[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 4; ++st) sA[kb][qb] = mfma16(ld_k(0, kb, st), qf[4 * qb + st], sA[kb][qb]);
      }
    if (NT == 1 && (nkeys & (KT - 1))) mask_ragged(0, sA);
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      m_run[qb] = true_max(sA, qb, m_run[qb]);
      if (PRE) {                                       // the loop's scores come out of the MFMA as S - m: bring S(0) to the same form
        set_negm(qb, m_run[qb]);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) sA[kb][qb][r] -= m_run[qb];
      }
    }
    for (int t = 0; t < NT; t += 4) {                  // iteration t reads K slot (t + 1) % 4 and V slot (t - 1) % 4
      iteration(t, sA, sB, pA, pB, std::integral_constant<int, 1>{}, std::integral_constant<int, 3>{});
      if (t + 1 < NT) iteration(t + 1, sB, sA, pB, pA, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
      if (t + 2 < NT) iteration(t + 2, sA, sB, pA, pB, std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});
      if (t + 3 < NT) iteration(t + 3, sB, sA, pB, pA, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
    }
    if (!(NT & 1)) {                                   // P(NT-1) lives in pA when the last iteration had even parity
      pA[0][0] = pB[0][0];
      pA[0][1] = pB[0][1];
      pA[1][0] = pB[1][0];
      pA[1][1] = pB[1][1];
    }
    {   // drain: PV(NT-1)
      const int vbase = V_OFF + ((NT - 1) % RV) * 16384;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          const bf16x8 f = ld_v(vbase, ks, db);
          o[db][0] = mfma16(f, pA[ks][0], o[db][0]);
          o[db][1] = mfma16(f, pA[ks][1], o[db][1]);
        }
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float l_tot = l_run[qb] + __shfl_xor(l_run[qb], 16, 64);
      l_tot += __shfl_xor(l_tot, 32, 64);
      const float inv = 1.0f / l_tot;
      const int qr = q_base + wave * 32 + 16 * qb + i16;
      if (SPLIT) {
        if (qr < A.q_rows) {
          float* op = A.part_o + ((size_t)sp * A.q_rows + qr) * row_stride + head * HD + 4 * g16;
#pragma unroll
          for (int db = 0; db < 8; ++db) *reinterpret_cast<f32x4*>(op + 16 * db) = o[db][qb] * inv;
          if (g16 == 0) A.part_lse[((size_t)sp * A.heads + head) * A.q_rows + qr] = m_run[qb] * A.scale + __logf(l_tot);
        }
      } else if (qr < q_lim) {
        unsigned short* op = A.out + (size_t)qr * A.ldo + head * HD + 4 * g16;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          u16x4 w4;
#pragma unroll
          for (int e = 0; e < 4; ++e) w4[e] = f2bf(o[db][qb][e] * inv);
          *reinterpret_cast<u16x4*>(op + 16 * db) = w4;
        }
        if (A.lse != nullptr && g16 == 0) A.lse[(size_t)head * A.q_rows + qr] = m_run[qb] * A.scale + __logf(l_tot);
      }
    }
    return;
  }

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float c2 = PRE ? 1.0f : A.scale_log2;     // the exponent forms are only launched when the product is 1 to rounding
  const int kswz = l31 & 15;
  const int vi = lane & 15, vg1 = (lane >> 4) & 1;
  const int v_rowq = vi >> 2;
  const int v_in = (vg1 << 5) | ((vi & 3) << 3);

  f32x16 s[2];
  bf16x8 pb[2][2];
  bf16x8 fA[4], fB[4];     // drain only
  // operand-fragment ring of the MFMA steps: RD slots of two fragments, LDS reads issued LA = RD - 1 batches (2 LA MFMAs) ahead.
  // Three slots in the phase-locked schedules (deeper measured slower there: 992 -> 946 TFLOP/s); six in the free-running one,
  // whose step trace showed every MFMA waiting for its own LDS round trip with reads only two batches ahead.
  constexpr int RD = FR == FR_FREE ? PP_RING : 3, LA = RD - 1;
  bf16x8 fr[RD][2];
  pb[0][0] = pb[0][1] = pb[1][0] = pb[1][1] = bf16x8{};      // P(-1) = 0 for the unconditional PV of tile 0
  if (PP_ABLATE) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fA[i] = fB[i] = bf16x8{};
    pb[0][0] = pb[0][1] = pb[1][0] = pb[1][1] = bf16x8{};
    s[0] = s[1] = f32x16{};
  }

  auto ldV = [&](bf16x8(&f)[4], const unsigned char* vb, int b, int s2) {
    if (PP_ABLATE & 4) return;
    const unsigned char* vr0 = vb + (32 * b + 16 * s2 + 4 * hi + v_rowq) * 256 + v_in;
    const unsigned char* vr1 = vr0 + 8 * 256;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ch = (d ^ v_rowq) << 6;
      const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr0 + ch));
      const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr1 + ch));
      f[d] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  };
  auto mmaV = [&](bf16x8(&f)[4], const bf16x8& p) {
    if (PP_ABLATE & 8) return;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[d], p, o[d], 0, 0, 0);
  };
#define PP_SB() __builtin_amdgcn_sched_barrier(0)

  // ---- step M(t): PV(t-1) then QK(t) = 16 batches of two MFMAs.  Operand fragments rotate through a three-slot
  //      ring of two fragments (24 VGPRs): the LDS reads of batch j+2 are issued before the MFMAs of batch j, so a
  //      read has two batches (~128 matrix-pipe cycles) to land.  (Four-fragment double buffering cost 8 VGPRs more,
  //      which is what did not fit next to O (64) + Q (32) + S (32) at three waves per SIMD.)
  //        PV batch j = (block b = j>>2, k-slot s2 = (j>>1)&1, d pair dh = j&1)     j = 0..7
  //        QK batch j = (block b = j>>2, k-steps 2*(j&3), 2*(j&3)+1)                 j = 0..7
  // phase: 0 = everything, 1 = only the first LA fragment reads (issued ahead of time), 2 = the rest (reads already issued)
  auto stepJ = [&](int t, int vt, auto j0c, auto j1c, auto phasec) {   // batches [J0, J1) of the list below, K from tile t, V from tile vt
    constexpr int J0 = decltype(j0c)::value, J1 = decltype(j1c)::value, PHASE = decltype(phasec)::value;
    const unsigned char* kb = smem + K_OFF + (t % RK) * 16384;
    const unsigned char* vb = smem + V_OFF + (vt % RV) * 16384;
    // lane-derived address terms are RECOMPUTED here from an opaque lane id (a handful of VALU ops): kept live across
    // the loop they were spilled at three waves per SIMD, and a scratch reload drains the DMA queue (shared vmcnt)
    int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(ln));
    const int hi = ln >> 5, l31 = ln & 31, kswz = ln & 15, v_rowq = (ln >> 2) & 3;
    const int v_in = (((ln >> 4) & 1) << 5) | ((ln & 3) << 3);
    auto load = [&](int j) {
      if (PP_ABLATE & 4) return;
      bf16x8(&f)[2] = fr[j % RD];
      if (j < 8) {
        const int bb = j >> 2, s2 = (j >> 1) & 1, dh = j & 1;
        const unsigned char* vr0 = vb + (32 * bb + 16 * s2 + 4 * hi + v_rowq) * 256 + v_in;
        const unsigned char* vr1 = vr0 + 8 * 256;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int ch = ((2 * dh + e) ^ v_rowq) << 6;
          const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr0 + ch));
          const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr1 + ch));
          f[e] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
      } else {
        const int q = j - 8, bb = q >> 2, ks0 = 2 * (q & 3);
        const unsigned char* krow = kb + (32 * bb + l31) * 256;
#pragma unroll
        for (int e = 0; e < 2; ++e)
          f[e] = *reinterpret_cast<const bf16x8*>(krow + (((2 * (ks0 + e) + hi) ^ kswz) << 4));
      }
    };
    auto mma = [&](int j) {
      if (PP_ABLATE & 8) return;
      bf16x8(&f)[2] = fr[j % RD];
      if (j < 8) {
        const int bb = j >> 2, s2 = (j >> 1) & 1, dh = j & 1;
#pragma unroll
        for (int e = 0; e < 2; ++e)
          o[2 * dh + e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[e], pb[bb][s2], o[2 * dh + e], 0, 0, 0);
      } else {
        const int q = j - 8, bb = q >> 2, ks0 = 2 * (q & 3);
        if ((q & 3) == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[bb][r] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) s[bb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[e], qf[ks0 + e], s[bb], 0, 0, 0);
      }
    };
    if (PHASE != 2) {
#pragma unroll
      for (int j = J0; j < J0 + LA && j < J1; ++j) load(j);
    }
    if (PHASE == 1) return;
#pragma unroll
    for (int j = J0; j < J1; ++j) {
      PP_SB();
      if (j + LA < J1) load(j + LA);
      mma(j);
    }
  };
  // PV(t-1) + QK(t).  At t == 0 there is no previous tile: P is all zero and the V fragments are read from tile 0, whose
  // DMA has landed — O += V^T * 0.  Unconditional on purpose: a branch here made the O accumulators a phi and cost
  // 32 v_mov_b64 per tile.
  using ic0 = std::integral_constant<int, 0>;
  using ic1 = std::integral_constant<int, 1>;
  using ic2 = std::integral_constant<int, 2>;
  using ic8 = std::integral_constant<int, 8>;
  using ic16 = std::integral_constant<int, 16>;
  auto stepM = [&](int t) { stepJ(t, t > 0 ? t - 1 : 0, ic0{}, ic16{}, ic0{}); };
  auto stepQK = [&](int t) { stepJ(t, 0, ic8{}, ic16{}, ic0{}); };
  auto prePV = [&](int t) { stepJ(t, t, ic0{}, ic8{}, ic1{}); };        // first V fragments, issued before the softmax
  auto stepPV = [&](int t) { stepJ(t, t, ic0{}, ic8{}, ic2{}); };

  // ---- step V(t): online softmax of the 64-key tile; P -> pb (bf16), in-place rescale of O when a max grew.
  //      Two halves (one per 32-key block of exponentials) so that the three-group schedule can put a phase
  //      boundary between them; with two groups they run back to back.
  pp_f32x2 v_mcv = {0.f, 0.f}, v_acc = {0.f, 0.f};
  const pp_f32x2 c2v = {c2, c2};
  auto exp_block = [&](int b) {
    // exponent arguments two at a time (v_pk_fma_f32); row sums in two plain chains
    float a0 = 0.f, a1 = 0.f;
#if !PP_PACKED
    const float mc = v_mcv[0];
#endif
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#if PP_PACKED
      const pp_f32x2 sv = {s[b][2 * i], s[b][2 * i + 1]};
      const pp_f32x2 e = sv * c2v - v_mcv;
      const float p0 = __builtin_amdgcn_exp2f(e[0]), p1 = __builtin_amdgcn_exp2f(e[1]);
#else
      const float p0 = __builtin_amdgcn_exp2f(s[b][2 * i] * c2 - mc);
      const float p1 = __builtin_amdgcn_exp2f(s[b][2 * i + 1] * c2 - mc);
#endif
      a0 += p0;
      a1 += p1;
      pb[b][i >> 2][(2 * i) & 7] = static_cast<__bf16>(p0);
      pb[b][i >> 2][(2 * i + 1) & 7] = static_cast<__bf16>(p1);
    }
    v_acc += pp_f32x2{a0, a1};
  };
  // Lazy reference maximum.  softmax is invariant to the exponent reference: p = exp2(c2*(s - M)) with ANY finite M
  // gives the same O / l as long as nothing overflows.  The true row maximum is computed for the first tile only;
  // later tiles reuse M (no 16-deep v_max3 chain, no cross-half exchange, no rescale factor — a third of the step's
  // VALU time, tools/trace_attn.sh) and only check the tile's row sums: if some row would exceed 2^20 (or overflowed
  // to inf), the tile is redone against its true maximum and O / l are rescaled.  m_run holds M; LSE = M*scale + ln l.
  constexpr float kLazyLimit = 1048576.f;
  auto tile_max = [&]() -> float {
    // first read of the S accumulators through a compiler-visible instruction (MFMA -> VALU wait states are not
    // inserted for inline-asm operands; a wave that arrives last at the barrier starts this step at once)
    float mx = attn_max3(__builtin_fmaxf(s[0][0], s[1][0]), m_run, m_run);
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = attn_max3(mx, s[0][r], s[1][r]);
    return attn_half_max(mx);
  };
  auto rescale_o = [&](float alpha) {
    asm volatile("" : "+v"(alpha));
    if (__any(alpha != 1.0f)) {
      asm volatile("s_nop 7" ::: "memory");          // hazards around inline-asm operands are padded by hand (rare path)
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(o[d][r]) : "v"(alpha));
      asm volatile("s_nop 3" ::: "memory");
    }
  };
  auto stepV1 = [&](int t) {
    // DMA of tile t+PD is issued HERE: an LDS-DMA instruction costs its issuing wave ~100+ cycles, which a
    // VALU step can afford and the MFMA step cannot
    if (FR == FR_PLAIN && loader && t + PD < NT && !(PP_ABLATE & 1)) issue(t + PD);
    if (t == NT - 1 && (nkeys & (KT - 1))) {     // ragged last tile (wave-uniform, executed once)
      const int kidx = t * KT + 4 * hi;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kidx + 32 * b + (r & 3) + 8 * (r >> 2) >= nkeys) s[b][r] = -INFINITY;
    }
    if (t == 0) m_run = tile_max();               // O and l are still zero: nothing to rescale
    const float mc = m_run * c2;
    v_mcv = pp_f32x2{mc, mc};
    v_acc = pp_f32x2{0.f, 0.f};
    exp_block(0);
  };
  auto stepV2 = [&](int t) {
    exp_block(1);
    float tile_sum = v_acc[0] + v_acc[1];
    if (__any(!(tile_sum < kLazyLimit))) {         // rare: this tile outgrew the reference (inf / NaN land here too)
      if (A.dbg_rescales != nullptr && lane == 0) atomicAdd(A.dbg_rescales, 1u);
      const float m_new = tile_max();              // >= m_run, identical in lane and lane^32
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
      m_run = m_new;
      const float mc = m_new * c2;
      v_mcv = pp_f32x2{mc, mc};
      v_acc = pp_f32x2{0.f, 0.f};
      exp_block(0);
      exp_block(1);
      tile_sum = v_acc[0] + v_acc[1];
      l_run *= alpha;
      rescale_o(alpha);
    }
    l_run += tile_sum;
  };
  auto phase_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  // ---- prologue: tiles 0 .. PD-1 in flight
  if (!SWP) {
#pragma unroll
    for (int i = 0; i < PD; ++i)
      if (loader && i < NT) issue(i);
  }

  if (SWP) {
    // ================= software-pipelined schedule (attn_variant 5; 6 = two four-wave workgroups per CU) =================================================
    // One wave keeps BOTH pipes busy by itself: iteration t interleaves, instruction by instruction, the 16 MFMAs of
    // PV(t-1), the 16 MFMAs of QK(t+1) and the ~110 VALU instructions of softmax(t) — three mutually independent streams
    // (P(t-1) and S(t) were finished last iteration, S(t+1) and P(t) are for the next one).  An MFMA holds the matrix pipe
    // for 32 cycles after issue; the wave uses them for the 3-4 VALU instructions placed behind it, so the wave-age
    // arbitration between the two waves of a SIMD (tools/probe_overlap.hip) no longer decides whether softmax and MFMA
    // overlap.  Costs: two S and two P register sets (parity-unrolled), K ring read one tile ahead, V ring one behind.
    f32x16 s2[2];
    bf16x8 pb2[2][2];
    pb2[0][0] = pb2[0][1] = pb2[1][0] = pb2[1][1] = bf16x8{};          // P(-1) = 0
    auto qk_plain = [&](int t, f32x16(&sx)[2]) {
      const unsigned char* kb = smem + K_OFF + (t % RK) * 16384;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sx[bb][r] = 0.f;
        const unsigned char* krow = kb + (32 * bb + l31) * 256;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
          sx[bb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(krow + (((2 * ks + hi) ^ kswz) << 4)),
                                                           qf[ks], sx[bb], 0, 0, 0);
      }
    };
    auto mask_ragged = [&](int t, f32x16(&sx)[2]) {
      // (opaque on purpose: the 32 comparisons below are loop-invariant lane masks — hipcc hoisted them out of the tile loop and kept
      //  64 scalar registers alive for a branch that one tile per work item takes; the scalars the loop does use — LDS slot addresses,
      //  row offsets of the K / V requests — were spilled to lanes and read back with v_readlane in front of every request)
      int kidx = t * KT + 4 * hi;
      asm volatile("" : "+v"(kidx));
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kidx + 32 * b + (r & 3) + 8 * (r >> 2) >= nkeys) sx[b][r] = -INFINITY;
    };
    auto true_max = [&](f32x16(&sx)[2], float floor_v) -> float {
      float mx = attn_max3(__builtin_fmaxf(sx[0][0], sx[1][0]), floor_v, floor_v);
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = attn_max3(mx, sx[0][r], sx[1][r]);
      return attn_half_max(mx);
    };
    auto exp_plain = [&](f32x16(&sx)[2], bf16x8(&px)[2][2], float mc) -> float {      // non-interleaved (tile 0 redo path)
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float p0 = __builtin_amdgcn_exp2f(sx[b][2 * i] * c2 - mc);
          const float p1 = __builtin_amdgcn_exp2f(sx[b][2 * i + 1] * c2 - mc);
          a0 += p0;
          a1 += p1;
          px[b][i >> 2][(2 * i) & 7] = static_cast<__bf16>(p0);
          px[b][i >> 2][(2 * i + 1) & 7] = static_cast<__bf16>(p1);
        }
      return a0 + a1;
    };
    // iteration t: sC = S(t) -> pC = P(t) (softmax), pP = P(t-1) -> O (PV), sN = S(t+1) (QK)
    // U4: lane terms of the fragment reads, once per kernel (K_OFF folded into the K terms; V_OFF = 0)
    f32x16 negm;                                       // PRE: -m in every element (MFMA C operand)
    auto set_negm = [&](float m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) negm[r] = -m;
      asm volatile("" : "+v"(negm));
    };
    if (PRE) set_negm(0.f);
    int kterm[8], vterm[4];
    if (CS) {
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        kterm[ks] = K_OFF + l31 * 256 + (((2 * ks + hi) ^ kswz) << 4);
        asm volatile("" : "+v"(kterm[ks]));
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        vterm[d] = (4 * hi + v_rowq) * 256 + v_in + ((d ^ v_rowq) << 6);
        asm volatile("" : "+v"(vterm[d]));
      }
    }
    auto body = [&](int t, f32x16(&sC)[2], f32x16(&sN)[2], bf16x8(&pC)[2][2], bf16x8(&pP)[2][2], auto kslot_c, auto vslot_c) -> float {
      constexpr int KSLOT = decltype(kslot_c)::value, VSLOT = decltype(vslot_c)::value;     // constant-slot forms only (-1 otherwise)
      const unsigned char* kb = smem + K_OFF + ((t + 1) % RK) * 16384;
      const unsigned char* vb = smem + V_OFF + ((t > 0 ? t - 1 : 0) % RV) * 16384;
#if PP_SWP_RECOMPUTE
      int ln = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      asm volatile("" : "+v"(ln));
      const int hi = ln >> 5, l31 = ln & 31, kswz = ln & 15, v_rowq = (ln >> 2) & 3;
      const int v_in = (((ln >> 4) & 1) << 5) | ((ln & 3) << 3);
#endif
      constexpr int RDs = PRE ? 2 : PP_SWP_RING, LAs = RDs - 1;  // fragment ring of this schedule (registers are tight; PRE spends 16 on negm)
      bf16x8 fs[RDs][2];
      auto load = [&](int j) {
        bf16x8(&f)[2] = fs[j % RDs];
        if (CS && j < 8) {
          const int bb = j >> 2, sl = (j >> 1) & 1, dh = j & 1;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const unsigned char* a0 = smem + vterm[2 * dh + e] + (VSLOT * 16384 + (32 * bb + 16 * sl) * 256);
            const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
            const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0 + 2048));
            f[e] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        } else if (CS) {
          const int q = j - 8, bb = q >> 2, ks0 = 2 * (q & 3);
#pragma unroll
          for (int e = 0; e < 2; ++e)
            f[e] = *reinterpret_cast<const bf16x8*>(smem + kterm[ks0 + e] + (KSLOT * 16384 + 32 * bb * 256));
        } else if (j < 8) {
          const int bb = j >> 2, sl = (j >> 1) & 1, dh = j & 1;
          const unsigned char* vr0 = vb + (32 * bb + 16 * sl + 4 * hi + v_rowq) * 256 + v_in;
          const unsigned char* vr1 = vr0 + 8 * 256;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int ch = ((2 * dh + e) ^ v_rowq) << 6;
            const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr0 + ch));
            const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(vr1 + ch));
            f[e] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
          }
        } else {
          const int q = j - 8, bb = q >> 2, ks0 = 2 * (q & 3);
          const unsigned char* krow = kb + (32 * bb + l31) * 256;
#pragma unroll
          for (int e = 0; e < 2; ++e) f[e] = *reinterpret_cast<const bf16x8*>(krow + (((2 * (ks0 + e) + hi) ^ kswz) << 4));
        }
      };
      auto mma1 = [&](int j, int e) {
        bf16x8(&f)[2] = fs[j % RDs];
        if (j < 8) {
          const int bb = j >> 2, sl = (j >> 1) & 1, dh = j & 1;
          o[2 * dh + e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[e], pP[bb][sl], o[2 * dh + e], 0, 0, 0);
        } else {
          const int q = j - 8, bb = q >> 2, ks0 = 2 * (q & 3);
          if (PRE && (q & 3) == 0 && e == 0) {
            sN[bb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[e], qf[ks0 + e], negm, 0, 0, 0);     // S - m
          } else {
            if ((q & 3) == 0 && e == 0) {
#pragma unroll
              for (int r = 0; r < 16; ++r) sN[bb][r] = 0.f;
            }
            sN[bb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[e], qf[ks0 + e], sN[bb], 0, 0, 0);
          }
        }
      };
      float p0 = 0.f, p1 = 0.f, e1 = 0.f;
      float acc4[4] = {0.f, 0.f, 0.f, 0.f};
      pp_f32x2 accp[2] = {pp_f32x2{0.f, 0.f}, pp_f32x2{0.f, 0.f}};
      u32x4 pw[2][2];                                  // P(t) as packed bf16 pairs: pw[b][half][k] = keys 2k, 2k+1 of that half
      const float mc = v_mcv[0];
#pragma unroll
      for (int j = 0; j < LAs; ++j) load(j);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int b = j >> 3, i = j & 7;               // softmax piece j = pair i of block b
        PP_SB();
#if PP_SWP_YIELD
        if ((j & 3) == 3 && wave < 4) __builtin_amdgcn_s_sleep(PP_SWP_YIELD);   // the older wave yields issue slots (experiment)
#endif
        if (j + LAs < 16 && !(PP_ABLATE & 4)) load(j + LAs);
        if (!(PP_ABLATE & 8)) mma1(j, 0);
        if (PP_ABLATE & 16) {                          // timing experiments: no transcendental
          p0 = __builtin_fmaf(sC[b][2 * i], c2, -mc);
          p1 = __builtin_fmaf(sC[b][2 * i + 1], c2, -mc);
        } else if (PP_SWP_PACKED) {                    // one v_pk_fma_f32 for the two exponent arguments
          const pp_f32x2 e2 = pp_f32x2{sC[b][2 * i], sC[b][2 * i + 1]} * c2v - v_mcv;
          p0 = __builtin_amdgcn_exp2f(e2[0]);
          p1 = __builtin_amdgcn_exp2f(e2[1]);
        } else if (PRE) {                              // the score is the exponent
          p0 = __builtin_amdgcn_exp2f(sC[b][2 * i]);
          e1 = sC[b][2 * i + 1];
        } else if (PP_SWP_BALANCE) {
          // the VALU work of a pair is split evenly around the second MFMA: two scale-FMAs + one exponential (24 cycles) here, the
          // other exponential + two adds + the pack (28 cycles) behind it — each piece fits under the 32 matrix-pipe cycles of the
          // OTHER wave's MFMA, where 40 + 12 left a bubble every pair
          p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sC[b][2 * i], c2, -mc));
          e1 = __builtin_fmaf(sC[b][2 * i + 1], c2, -mc);
          asm volatile("" : "+v"(e1));
        } else {
          p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sC[b][2 * i], c2, -mc));
          p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(sC[b][2 * i + 1], c2, -mc));
        }
        PP_SB();
        if (!(PP_ABLATE & 8)) mma1(j, 1);
        if ((PRE || PP_SWP_BALANCE) && !PP_SWP_PACKED && !(PP_ABLATE & 16)) p1 = __builtin_amdgcn_exp2f(e1);
        if (!(PP_ABLATE & 64)) {                       // four independent row-sum chains, pinned behind this MFMA
          if (PP_SWP_PACKED) {
            pp_f32x2& a2 = (j & 1) ? accp[1] : accp[0];
            const pp_f32x2 pv = {p0, p1};
            asm volatile("s_nop 0\n\tv_pk_add_f32 %0, %0, %1" : "+v"(a2) : "v"(pv));
          } else {
            // p0 / p1 come straight out of v_exp_f32: a VALU instruction that reads a transcendental's result needs one wait state
            // behind it, and the hazard recogniser does not look into inline asm.  Latent until a recompile puts the exponential
            // directly in front of this add: seen as -inf row sums in lanes 0-3 of every 8 in a build with a loop around the kernel body.
            asm volatile("s_nop 0\n\tv_add_f32 %0, %0, %1" : "+v"(acc4[(2 * j) & 3]) : "v"(p0));
            asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc4[(2 * j + 1) & 3]) : "v"(p1));
          }
        }
        if (!(PP_ABLATE & 32)) {
          unsigned pk;
          asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(p0), "v"(p1));
          pw[b][i >> 2][i & 3] = pk;
        } else if (j == 0) {
          pw[0][0][0] = __builtin_bit_cast(unsigned, p0);
        }
      }
      PP_SB();
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) pC[b][h2] = __builtin_bit_cast(bf16x8, pw[b][h2]);
      if (PP_SWP_PACKED) return (accp[0][0] + accp[0][1]) + (accp[1][0] + accp[1][1]);
      return (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    };
    auto iteration = [&](int t, f32x16(&sC)[2], f32x16(&sN)[2], bf16x8(&pC)[2][2], bf16x8(&pP)[2][2], auto kslot_c, auto vslot_c) {
      long long tr[6] = {0, 0, 0, 0, 0, 0};
      if (PP_TRACE) tr[0] = __builtin_readcyclecounter();
      if (DUAL) {
        // issue order per iteration: K(t+2) then V(t+1) (4 pieces each per wave).  Here K(t+1) must have landed; the V(t) pieces
        // issued after it may stay in flight (PV(t) is next iteration's) — except at t = 0, where K(1) was the last thing issued
        if (t == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        // own pieces of tile t+1 landed (t+2 may stay in flight); only waves 0-3 have any (8 per tile, see below)
        if (t + 2 < NT) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (PP_TRACE) tr[1] = __builtin_readcyclecounter();
      __builtin_amdgcn_s_barrier();                    // tile t+1 complete for everyone; K(t) and V(t-2) are free
      if (PP_TRACE) tr[2] = __builtin_readcyclecounter();
      // (the four pieces were also tried behind MFMAs 2 / 6 / 10 / 14 of the body: 1045 -> 991 TFLOP/s — an LDS-DMA
      //  instruction stalls its wave for ~100 cycles and inside the body that stall also holds back the wave's MFMAs)
      // LDS-DMA issue stalls a wave for ~80 cycles per instruction: the OLDER wave of each SIMD issues the pieces of both
      // (8 per tile) while the younger one starts the matrix pipe at once — which also staggers the two waves' bodies
      if (DUAL) {
        if (t + 2 < NT) {
          issue_w(t + 2, wave, 1);
          issue_w(t + 2, wave + 4, 1);
        }
        if (t + 1 < NT) {
          issue_w(t + 1, wave, 2);
          issue_w(t + 1, wave + 4, 2);
        }
      } else if (U4) {
        if (wave < 4) {                                  // K three tiles ahead, V two: four slots each
          if (t + 3 < NT) {
            issue_w(t + 3, wave, 1);
            issue_w(t + 3, wave + 4, 1);
          }
          if (t + 2 < NT) {
            issue_w(t + 2, wave, 2);
            issue_w(t + 2, wave + 4, 2);
          }
        }
      } else if (wave < 4 && t + PD < NT && !(PP_ABLATE & 1)) {
        issue_w(t + PD, wave);
        issue_w(t + PD, wave + 4);
      }
      if (PP_TRACE) tr[3] = __builtin_readcyclecounter();
      if (t == NT - 1 && (nkeys & (KT - 1))) mask_ragged(t, sC);
      const float mc0 = m_run * c2;
      v_mcv = pp_f32x2{mc0, mc0};
      float tile_sum = body(t, sC, sN, pC, pP, kslot_c, vslot_c);
      if (PP_TRACE) {
        asm volatile("" ::"v"(tile_sum), "v"(sN[1][15]), "v"(o[3][15]));
        tr[4] = __builtin_readcyclecounter();
      }
      if (PRE) {
        if (__any(!(tile_sum < kLazyLimit))) {         // rare: sC holds S(t) - m_run, sN already holds S(t+1) - m_run
          if (A.dbg_rescales != nullptr && lane == 0) atomicAdd(A.dbg_rescales, 1u);
          const float d = true_max(sC, 0.f);           // >= 0: how far this tile's maximum lies above the reference
          const float alpha = __builtin_amdgcn_exp2f(-d);
          tile_sum = exp_plain(sC, pC, d);
          m_run += d;
          l_run *= alpha;
          rescale_o(alpha);
          set_negm(m_run);
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) sN[b][r] -= d;
        }
      } else if (__any(!(tile_sum < kLazyLimit))) {    // rare: this tile outgrew the reference maximum
        if (A.dbg_rescales != nullptr && lane == 0) atomicAdd(A.dbg_rescales, 1u);
        const float m_new = true_max(sC, m_run);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c2);
        m_run = m_new;
        tile_sum = exp_plain(sC, pC, m_new * c2);
        l_run *= alpha;
        rescale_o(alpha);
      }
      l_run += tile_sum;
      if (PP_TRACE && t < 48 && lane == 0) {           // stamps of the first 48 tiles, staged in LDS behind the rings
        long long* tp = reinterpret_cast<long long*>(smem + LDS_SWP) + (t * 8 + wave) * 8;
        tr[5] = __builtin_readcyclecounter();
#pragma unroll
        for (int i = 0; i < 6; ++i) tp[i] = tr[i];
      }
    };
    if (U6) {                                          // V slot 2 is read (times P(-1) = 0) by the PV of iteration 0: clear it (256 threads x 64 B)
#pragma unroll
      for (int z = 0; z < 4; ++z) *reinterpret_cast<u32x4*>(smem + V_OFF + 2 * 16384 + tid * 64 + z * 16) = u32x4{0, 0, 0, 0};
    }
    if (DUAL) {                                        // K(0), V(0), K(1); K(0) and V(0) must land before QK(0) / the P = 0 pass over V(0)
      issue_w(0, wave, 3);
      issue_w(0, wave + 4, 3);
      if (NT > 1) {
        issue_w(1, wave, 1);
        issue_w(1, wave + 4, 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    if (U4) {
      // V slot 3 is read (times P(-1) = 0) by the PV of iteration 0 before anything was copied there: LDS starts with arbitrary bits
      *reinterpret_cast<u32x4*>(smem + V_OFF + 3 * 16384 + tid * 32) = u32x4{0, 0, 0, 0};
      *reinterpret_cast<u32x4*>(smem + V_OFF + 3 * 16384 + tid * 32 + 16) = u32x4{0, 0, 0, 0};
      if (wave < 4) {                                   // K(0), V(0), K(1), V(1), K(2): everything but K(2) has to land now
        issue_w(0, wave, 3);
        issue_w(0, wave + 4, 3);
        if (NT > 1) {
          issue_w(1, wave, 3);
          issue_w(1, wave + 4, 3);
        }
        if (NT > 2) {
          issue_w(2, wave, 1);
          issue_w(2, wave + 4, 1);
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
    }
#pragma unroll
    for (int i = 0; i < PD; ++i)
      if (!DUAL && !U4 && i < NT && wave < 4) {
        issue_w(i, wave);
        issue_w(i, wave + 4);
      }
    if (!DUAL && !U4) {
      const int fl = min(NT, PD) - 1;                  // tiles that may stay in flight behind tile 0 (8 pieces each)
      if (fl <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (fl == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    qk_plain(0, s);
    if (NT == 1 && (nkeys & (KT - 1))) mask_ragged(0, s);
    m_run = true_max(s, m_run);
    if (PRE) {                                         // the loop's scores come out of the MFMA as S - m: bring S(0) to the same form
      set_negm(m_run);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[b][r] -= m_run;
    }
    using ic = std::integral_constant<int, -1>;
    if (U4) {                                          // iteration t reads K slot (t + 1) % 4 and V slot (t - 1) % 4
      for (int t = 0; t < NT; t += 4) {
        iteration(t, s, s2, pb, pb2, std::integral_constant<int, 1>{}, std::integral_constant<int, 3>{});
        if (t + 1 < NT) iteration(t + 1, s2, s, pb2, pb, std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{});
        if (t + 2 < NT) iteration(t + 2, s, s2, pb, pb2, std::integral_constant<int, 3>{}, std::integral_constant<int, 1>{});
        if (t + 3 < NT) iteration(t + 3, s2, s, pb2, pb, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
      }
    } else if (U6) {                                   // K slot (t + 1) % 2, V slot (t + 2) % 3
      for (int t = 0; t < NT; t += 6) {
        iteration(t, s, s2, pb, pb2, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
        if (t + 1 < NT) iteration(t + 1, s2, s, pb2, pb, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        if (t + 2 < NT) iteration(t + 2, s, s2, pb, pb2, std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
        if (t + 3 < NT) iteration(t + 3, s2, s, pb2, pb, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
        if (t + 4 < NT) iteration(t + 4, s, s2, pb, pb2, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
        if (t + 5 < NT) iteration(t + 5, s2, s, pb2, pb, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
      }
    } else {
      for (int t = 0; t < NT; t += 2) {
        iteration(t, s, s2, pb, pb2, ic{}, ic{});
        if (t + 1 < NT) iteration(t + 1, s2, s, pb2, pb, ic{}, ic{});
      }
    }
    if (NT & 1) {                                      // P(NT-1) lives in pb when the last iteration had even parity
    } else {
      pb[0][0] = pb2[0][0];
      pb[0][1] = pb2[0][1];
      pb[1][0] = pb2[1][0];
      pb[1][1] = pb2[1][1];
    }
    if (DUAL) {                                        // V(NT-1) was allowed to stay in flight; everyone's pieces must be visible
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    {   // drain: PV(NT-1)
      const unsigned char* vb = smem + V_OFF + ((NT - 1) % RV) * 16384;
      ldV(fA, vb, 0, 0);
      ldV(fB, vb, 0, 1);
      PP_SB();
      mmaV(fA, pb[0][0]);
      ldV(fA, vb, 1, 0);
      PP_SB();
      mmaV(fB, pb[0][1]);
      ldV(fB, vb, 1, 1);
      PP_SB();
      mmaV(fA, pb[1][0]);
      mmaV(fB, pb[1][1]);
    }
  } else if (FR == FR_FREE) {
    for (int t = 0; t < NT; ++t) {
      long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
      if (PP_TRACE) tr[0] = __builtin_readcyclecounter();
      pp_wait_tiles(min(NT - 1 - t, PD - 1));          // own pieces of tile t landed (t+1 may stay in flight)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (PP_TRACE) tr[1] = __builtin_readcyclecounter();
      __builtin_amdgcn_s_barrier();                    // tile t complete for everyone; everyone is done with tile t-1
      if (PP_TRACE) tr[2] = __builtin_readcyclecounter();
      // an LDS-DMA instruction stalls its issuing wave for ~100 cycles: the older wave of each SIMD issues its pieces now,
      // while the younger one starts the matrix pipe, and the younger one after its QK, while the older one computes
      if (wave < 4 && t + PD < NT && !(PP_ABLATE & 1)) issue(t + PD);
      if (PP_TRACE) tr[3] = __builtin_readcyclecounter();
      stepQK(t);
      if (wave >= 4 && t + PD < NT && !(PP_ABLATE & 1)) issue(t + PD);
      prePV(t);
      if (PP_TRACE) {
        asm volatile("" ::"v"(s[1][15]));
        tr[4] = __builtin_readcyclecounter();
      }
      if (!(PP_ABLATE & 2)) {
        stepV1(t);
        stepV2(t);
      }
      if (PP_TRACE) {
        asm volatile("" ::"v"(l_run), "v"(pb[1][1]));
        tr[5] = __builtin_readcyclecounter();
      }
      stepPV(t);
      if (PP_TRACE && t < 64 && lane == 0) {
        asm volatile("" ::"v"(o[3][15]));
        long long* tp = reinterpret_cast<long long*>(smem + LDS_BYTES) + (t * 8 + wave) * 8;
        tr[6] = __builtin_readcyclecounter();
#pragma unroll
        for (int i = 0; i < 7; ++i) tp[i] = tr[i];
      }
    }
  } else if (NG == 2) {
    // barrier index :   2t            2t+1          2t+2
    // G0            :   M(t)          V(t)          M(t+1)
    // G1            :   V(t-1)        M(t)          V(t)
    if (grp == 1) {                                   // phase shift: G1 runs one barrier behind G0
      pp_wait_tiles(min(NT, PD) - 1);
      __builtin_amdgcn_s_barrier();
    }
    for (int t = 0; t < NT; ++t) {
      long long tr[7] = {0, 0, 0, 0, 0, 0, 0};
      if (PP_TRACE) tr[0] = __builtin_readcyclecounter();
      if (grp == 0) pp_wait_tiles(min(NT - 1 - t, PD - 1));   // own pieces of tile t landed (t+1 may stay in flight)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (PP_TRACE) tr[1] = __builtin_readcyclecounter();
      __builtin_amdgcn_s_barrier();
      if (PP_PRIO == 1) __builtin_amdgcn_s_setprio(1);
      if (PP_TRACE) tr[2] = __builtin_readcyclecounter();
      stepM(t);
      if (PP_TRACE) tr[3] = __builtin_readcyclecounter();
      if (PP_PRIO == 1) __builtin_amdgcn_s_setprio(0);
      if (grp == 1 && t + 1 < NT) pp_wait_tiles(max(min(NT - 2 - t, PD - 2), 0));   // tile t+1 before G0's M(t+1)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (PP_TRACE) tr[4] = __builtin_readcyclecounter();
      __builtin_amdgcn_s_barrier();
      if (PP_TRACE) tr[5] = __builtin_readcyclecounter();
      if (PP_PRIO == 2) __builtin_amdgcn_s_setprio(3);
      if (!(PP_ABLATE & 2)) {
        stepV1(t);
        stepV2(t);
      }
      if (PP_PRIO == 2) __builtin_amdgcn_s_setprio(0);
      if (PP_TRACE && t < 64 && lane == 0) {           // stamps go to LDS (no VMEM traffic inside the loop)
        long long* tp = reinterpret_cast<long long*>(smem + LDS_BYTES) + (t * 8 + wave) * 8;
        tr[6] = __builtin_readcyclecounter();
#pragma unroll
        for (int i = 0; i < 7; ++i) tp[i] = tr[i];
      }
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();        // balance the phase shift
  } else {
    // Three groups, one phase apart; phase p is opened by barrier B_p, group g runs its local phase p - g:
    //   B index :  3t       3t+1     3t+2     3t+3     3t+4
    //   G0      :  M(t)     V1(t)    V2(t)    M(t+1)   V1(t+1)
    //   G1      :  V2(t-1)  M(t)     V1(t)    V2(t)    M(t+1)
    //   G2      :  V1(t-1)  V2(t-1)  M(t)     V1(t)    V2(t)
    // -> every phase has exactly one group on the matrix pipe and two groups sharing the VALU.
    // Tile t (K for QK(t), V for PV(t) one tile later) must be complete at B_3t, the barrier before G0's M(t): the
    // loader waves of G0 retire their pieces just before it at the top of their iteration t, those of G1 before
    // the same barrier between their V1(t-1) and V2(t-1).  Ring slot of K(t+PD) = slot of K(t-1), last read by G2's
    // M(t-1) in phase 3t-1; it is refilled by G0 in phase 3t+1 and by G1 in phase 3t+2.  (V: slot of V(t-2), same.)
    if (grp >= 1) {
      if (loader) pp_wait_tiles(min(NT, PD) - 1);      // B_0 publishes tile 0
      __builtin_amdgcn_s_barrier();
    }
    if (grp == 2) __builtin_amdgcn_s_barrier();
    for (int t = 0; t < NT; ++t) {
      long long tr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (PP_TRACE) tr[0] = __builtin_readcyclecounter();
      if (grp == 0) pp_wait_tiles(min(NT - 1 - t, PD - 1));
      phase_barrier();
      if (PP_PRIO == 1) __builtin_amdgcn_s_setprio(2);
      if (PP_TRACE) tr[1] = __builtin_readcyclecounter();
      stepM(t);
      if (PP_TRACE) tr[2] = __builtin_readcyclecounter();
      if (PP_PRIO == 1) __builtin_amdgcn_s_setprio(0);
      phase_barrier();
      if (PP_PRIO == 2) __builtin_amdgcn_s_setprio(3);
      if (PP_TRACE) tr[3] = __builtin_readcyclecounter();
      if (!(PP_ABLATE & 2)) stepV1(t);
      if (grp == 1 && t + 1 < NT) pp_wait_tiles(min(NT - 2 - t, PD - 1));   // own pieces of tile t+1 (B_3(t+1) is next)
      if (PP_TRACE) {
        asm volatile("" ::"v"(v_acc));
        tr[4] = __builtin_readcyclecounter();
      }
      phase_barrier();
      if (PP_TRACE) tr[5] = __builtin_readcyclecounter();
      if (!(PP_ABLATE & 2)) stepV2(t);
      if (PP_PRIO == 2) __builtin_amdgcn_s_setprio(0);
      if (PP_TRACE && t < 64 && lane == 0) {
        asm volatile("" ::"v"(l_run), "v"(pb[1][1]));
        long long* tp = reinterpret_cast<long long*>(smem + LDS_BYTES) + (t * 12 + wave) * 8;
        tr[6] = __builtin_readcyclecounter();
#pragma unroll
        for (int i = 0; i < 7; ++i) tp[i] = tr[i];
      }
    }
    if (grp <= 1) __builtin_amdgcn_s_barrier();        // balance the phase shifts
    if (grp == 0) __builtin_amdgcn_s_barrier();
  }
  if (PP_TRACE && wi == 0 && A.lse != nullptr) {
    __syncthreads();
    const long long* tp = reinterpret_cast<const long long*>(smem + (SWP ? LDS_SWP : LDS_BYTES));
    for (int i = tid; i < (SWP ? 48 : 64) * 4 * NG * 8; i += 256 * NG) reinterpret_cast<long long*>(A.lse)[i] = tp[i];
  }
  // ---- drain: PV of the last tile
  if (FR == FR_PLAIN) {
    const unsigned char* vb = smem + V_OFF + ((NT - 1) % RV) * 16384;
    ldV(fA, vb, 0, 0);
    ldV(fB, vb, 0, 1);
    PP_SB();
    mmaV(fA, pb[0][0]);
    ldV(fA, vb, 1, 0);
    PP_SB();
    mmaV(fB, pb[0][1]);
    ldV(fB, vb, 1, 1);
    PP_SB();
    mmaV(fA, pb[1][0]);
    mmaV(fB, pb[1][1]);
  }
#undef PP_SB

  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  if (SPLIT) {
    if (qrow < A.q_rows) {
      float* op = A.part_o + ((size_t)sp * A.q_rows + qrow) * row_stride + head * HD + 4 * hi;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = o[d][4 * g + e] * inv;
          *reinterpret_cast<f32x4*>(op + 32 * d + 8 * g) = w;
        }
      if (hi == 0) A.part_lse[((size_t)sp * A.heads + head) * A.q_rows + qrow] = m_run * A.scale + __logf(l_tot);
    }
    return;
  }
  if (qrow < q_lim) {
    unsigned short* op = A.out + (size_t)qrow * A.ldo + head * HD + 4 * hi;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = f2bf(o[d][4 * g + e] * inv);
        *reinterpret_cast<u16x4*>(op + 32 * d + 8 * g) = w;
      }
    if (A.lse != nullptr && hi == 0 && !PP_TRACE) A.lse[(size_t)head * A.q_rows + qrow] = m_run * A.scale + __logf(l_tot);
  }
}

#if !PP_MULTI      // (the rest of the file: the merge kernel and the launchers of attn_fwd_pp_kernel)
// out[row][head][:] = sum_s w_s * part_o[s][row][head][:],  w_s = exp(lse_s - LSE) ; LSE = log sum_s exp(lse_s)
// (the same algebra as ifx_lse_merge, over `splits` fp32 partials, rounded to bf16 once)
__global__ __launch_bounds__(256) void attn_split_merge_kernel(const float* __restrict__ part_o,
                                                               const float* __restrict__ part_lse,
                                                               unsigned short* __restrict__ out, float* __restrict__ lse,
                                                               int q_rows, int heads, int splits, int ldo) {
  const int pair = blockIdx.x * 8 + (threadIdx.x >> 5);      // (row, head) pair, 32 lanes x 4 channels
  if (pair >= q_rows * heads) return;
  const int row = pair / heads, head = pair - row * heads, c = (threadIdx.x & 31) * 4;
  // four slots per pass: their LSE values and partial rows are requested together (a run-time loop of dependent load -> use steps pays
  // one memory latency per slot: 12.9 us for 585 rows x 12 heads x 5 slots); the accumulation order stays slot 0, 1, 2, ...
  float mx = -INFINITY;
  for (int s0 = 0; s0 < splits; s0 += 4) {
    float l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) l[u] = s0 + u < splits ? part_lse[((size_t)(s0 + u) * heads + head) * q_rows + row] : -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) mx = fmaxf(mx, l[u]);
  }
  float den = 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < splits; s0 += 4) {
    float l[4];
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = min(s0 + u, splits - 1);
      l[u] = part_lse[((size_t)s * heads + head) * q_rows + row];
      v[u] = *reinterpret_cast<const f32x4*>(part_o + (((size_t)s * q_rows + row) * heads + head) * 128 + c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s0 + u < splits) {
        const float w = __expf(l[u] - mx);
        den += w;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += w * v[u][e];
      }
    }
  }
  const float inv = 1.0f / den;
  u16x4 w4;
#pragma unroll
  for (int e = 0; e < 4; ++e) w4[e] = f2bf(acc[e] * inv);
  *reinterpret_cast<u16x4*>(out + (size_t)row * ldo + head * 128 + c) = w4;
  if (lse != nullptr && c == 0) lse[(size_t)head * q_rows + row] = mx + __logf(den);
}

// One launcher for every (NG, FR) instantiation group.  `paged`: 0 contiguous, 1 wave-uniform page translation, 2 per-lane translation —
// page geometries whose request pieces may straddle pages (page_size % 4 != 0, unaligned range starts, one-row pages ...), built for
// the plain two-group schedule only (the plan routes such views there).  Each kernel of a group opts into its dynamic LDS on its own
// first use on a device (launch_lds, ifx_launch.h).
template <int NG, int FR>
static int launch_pp(const AttnArgsPP& a, int paged, bool split, dim3 grid, int lds, hipStream_t stream) {
  auto launch = [&](auto kind) {
    constexpr int P = decltype(kind)::value;
    const char* const what = "ifx_attn_fwd_paged(pp)";
    return split ? launch_lds<attn_fwd_pp_kernel<P, true, NG, FR>>(grid, dim3(NG * 256), lds, stream, what, a)
                 : launch_lds<attn_fwd_pp_kernel<P, false, NG, FR>>(grid, dim3(NG * 256), lds, stream, what, a);
  };
  if constexpr (NG == 2 && FR == pp::FR_PLAIN) {
    if (paged == 2) return launch(std::integral_constant<int, 2>{});
  }
  return paged ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 0>{});
}

static void launch_merge(const float* part_o, const float* part_lse, unsigned short* out, float* lse, int q_rows, int heads, int splits,
                         int ldo, hipStream_t stream) {
  const int pairs = q_rows * heads;
  hipLaunchKernelGGL(attn_split_merge_kernel, dim3((pairs + 7) / 8), dim3(256), 0, stream, part_o, part_lse, out, lse, q_rows, heads,
                     splits, ldo);
}

// Launches what attn_plan (ifx_attn.hip) worked out: schedule `s`, in its exponent form when `pre`, then — for a self-contained split
// launch (a.out given) — the merge of its partials.  Loop form and LDS size come from THIS file's row of the table, the one its
// kernels were compiled with (a lab build may give PP_PD, PP_TRACE or PP_DUAL_FR to this file alone).
int launch_attn_pp(const AttnArgsPP& a, const AttnSchedule& s, int paged, bool write_partials, AttnForm form, dim3 grid, hipStream_t stream) {
  using namespace pp;
  const AttnSchedule& own = attn_schedule(s.variant);
  int fr = form.pre ? own.fr_pre : own.fr;
  if (form.mfma16) {
    if (fr != FR_U4 && fr != FR_U4_PRE) {
      set_error("ifx_attn_fwd_paged(pp): the 16x16x32 form is built for the constant-slot loop of variant 7 only (not variant %d)", s.variant);
      return IFX_EUNSUP;
    }
    fr = fr == FR_U4 ? FR_U4_M16 : FR_U4_PRE_M16;
  }
  if (paged == 2 && !(own.ng == 2 && fr == FR_PLAIN)) {
    set_error("ifx_attn_fwd_paged(pp): per-lane page translation is built for the plain two-group schedule only (not variant %d)", s.variant);
    return IFX_EUNSUP;
  }
#define PP_CASE(NG, FR) \
  case (NG) * 16 + (FR): rc = launch_pp<NG, FR>(a, paged, write_partials, grid, own.lds_bytes, stream); break
  int rc = IFX_OK;
  switch (own.ng * 16 + fr) {
    PP_CASE(1, FR_U6_DUAL_PRE);
    PP_CASE(1, PP_DUAL_FR);
    PP_CASE(2, FR_SWP);
    PP_CASE(2, FR_U4_PRE);
    PP_CASE(2, FR_U4);
    PP_CASE(2, FR_U4_PRE_M16);
    PP_CASE(2, FR_U4_M16);
    PP_CASE(2, FR_FREE);
    PP_CASE(3, FR_PLAIN);
    PP_CASE(2, FR_PLAIN);
    default:
      set_error("ifx_attn_fwd_paged(pp): no kernel built for %d wave groups in loop form %d", own.ng, fr);
      return IFX_EUNSUP;
  }
#undef PP_CASE
  if (rc != IFX_OK) return rc;
  if (a.splits > 1 && a.out != nullptr) launch_merge(a.part_o, a.part_lse, a.out, a.lse, a.q_rows, a.heads, a.splits, a.ldo, stream);
  return check_launch("ifx_attn_fwd_paged(pp)");
}

int launch_attn_merge(const float* workspace, int slot_cap, int slots_used, unsigned short* out, float* lse, int q_rows,
                      int heads, hipStream_t stream, int ldo) {
  launch_merge(workspace, workspace + (size_t)slot_cap * q_rows * heads * 128, out, lse, q_rows, heads, slots_used,
               ldo > 0 ? ldo : heads * 128, stream);
  return check_launch("ifx_attn_merge_partials");
}

#endif  // !PP_MULTI

}  // namespace ifx

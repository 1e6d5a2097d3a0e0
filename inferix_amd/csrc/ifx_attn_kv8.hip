// Self-attention over an 8-bit (OCP e4m3) KV cache on v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales (gfx950), and the row kernel
// that fills that cache.  Entry points and the numeric contract: include/inferix_hip_kv8.h.  Launch plan and LDS layout: ifx_attn_kv8.h.
//
// attn_fwd_kv8_kernel: 256 query rows x one head per workgroup, 8 waves x 32 rows, keys in tiles of 64.
//   * S^T = K q^T.  A = a 32-key block of the K tile, B = the wave's q rows (in registers for the whole launch), two K = 64 steps over
//     the 128 channels.  Both operands are read with the same lane -> byte map (row lane & 31, bytes [32 (lane >> 5), +32) of a 64-byte
//     step), which is all the Q8 GEMM tile of ifx_gemm_pp.hip relies on too: register byte j of lane half h is the same contraction
//     index in A and in B, whatever order the hardware gives them.
//   * The accumulator of a 32x32 block holds, in lane (n, h) = (lane & 31, lane >> 5), query row n and keys 8 g + 4 h + e of register
//     4 g + e (the layout the Q8 GEMM's epilogue uses).  A lane's 2 x 16 scores of a tile are therefore exactly the 32 bytes of a B operand
//     of the PV product O^T = V^T P^T once byte j = 16 kb + 4 g + e of half h is DEFINED to be key 32 kb + 8 g + 4 h + e: exp2 goes
//     straight from the accumulator through v_cvt_pk_fp8_f32 into the operand registers, P never touches LDS.
//   * V^T in that key order is made by a transposing stage: every thread loads 4 keys x 4 channels of the V tile (one dword per key,
//     zeros past kv_len through the buffer bound), transposes the 4 x 4 bytes with v_perm_b32 and stores four dwords — one channel, four
//     consecutive keys, which the order above keeps adjacent — into the slot's V^T rows.  A = 32 channel rows of V^T, 4 blocks.
//   * K tiles arrive by LDS-DMA (one 1 KiB piece per wave and tile, the chunk swizzle of the Q8 GEMM tile).  Ring of 3 slots, one
//     barrier per tile: while tile t is multiplied, V^T of t + 1 has just been stored and K / V of t + 2 are in flight.
//   * C operand of a score block's first MFMA is 7 - m (m: the row's lazy maximum), so the accumulator is the exp2 argument.  When a
//     tile's largest argument exceeds 8.75 (2^8.75 = 431 < 448) the wave shifts m, the tile's arguments, O and the row sum.
#include "ifx_attn_kv8_multi.h"
#include "ifx_launch.h"
#include "ifx_lds_dma.h"
#include "ifx_rows.h"

namespace ifx {
namespace {
using namespace kv8;

typedef int v8i __attribute__((ext_vector_type(8)));

struct AttnKv8Args {
  const unsigned char* q;
  int ldq;
  unsigned short* out;
  int ldo;
  float* lse;
  const unsigned char *k, *v;
  const float* v_scale;
  int q_rows, group, pitch, kv_start, kv_len, row_tiles, total, per_xcd;
};

__device__ __forceinline__ v8i cat(v4i lo, v4i hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ f32x16 mfma8(v8i a, v8i b, f32x16 c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}
// device memory that no launch on the way writes, read through the constant address space: a wave-uniform address is a scalar load
typedef const float __attribute__((address_space(4))) * const_f32_ptr;
__device__ __forceinline__ f32x16 splat16(float x) { return f32x16{x, x, x, x, x, x, x, x, x, x, x, x, x, x, x, x}; }

// Row tile `tile` of head `head` of the launch A describes: the whole workgroup, from the q fragments to the stores.  All kernels
// below end in it; `head` and `tile` are workgroup-uniform.  kPartial (the split-key launch): A's key range is ONE CHUNK's, and the
// epilogue leaves the rows unnormalised in `part`, fp32 [row_tiles][8 waves][kPartWave] (ifx_attn_kv8.h), instead of writing out / lse; no
// thread returns early, the caller has barriers to come.
//
// kGrouped (the ring cache's launch, include/inferix_hip_kv8_ring.h): the keys are slots [0, kv_len) in groups of W.tokens slots, A.v_scale
// is the table [group][kv_head], and the walk along the keys is per group — tile t is tile t % tpg of group t / tpg and starts at slot
// g * tokens + 64 j, so that a tile's V rows share one scale.  Two scalar cursors follow the walk, the loader's two tiles ahead of the
// compute loop's; neither divides.  A group's last tile runs into the next group's rows when tokens % 64 != 0: those keys get -inf by
// index (P = 0 exactly; the V bytes there are live rows of the next group or the zeros of the descriptor bound).  O is kept in units of
// the CURRENT group's scale: entering a group whose scale differs, every lane multiplies its accumulators by old / new (exact for
// powers of two); the row sum and the lazy maximum do not see V.
//
// kPartial && kGrouped (the grouped split-key launch, include/inferix_hip_kv8_ring_split.h): W.nt tiles of the walk from the tile S0
// names, which may be any tile of any group, so a chunk can begin and end inside a group.  Both cursors and the scale pointer start at
// S0; the rest of the walk is the grouped launch's (the descriptor bound stays A.kv_len, the end of the WHOLE walk).  The partial O
// is left in units of `vs`, the scale of the group of the chunk's last tile.
struct GroupWalk {
  int tokens, tpg, nt, kv_heads;      // slots per group, ceil(tokens / 64), tiles of the whole walk, row length of the scale table
};
struct GroupStart {
  int g, j, row;                      // a chunk's first tile: tile j of group g, which starts at slot row = g * tokens + 64 j
};
// kSeg (the ranges launch over a two-segment key map, include/inferix_hip_kv8_magi.h): the keys are two runs of consecutive slots,
// [a0, a1) then [b0, b1), either of which may be empty; A.kv_start / A.kv_len are not read.  The tile list is CUT where the first run
// ends: ceil((a1 - a0) / 64) tiles counted from a0, then the tiles of the second run counted from b0.  A tile's base slot, its run's
// end (the index mask of the run's last tile: P = 0 exactly) and the descriptor bound that zeroes K / V rows past that end are chosen
// per tile by t < nta: scalar selects, so every tile is addressed wave-uniformly and nothing of the other run, or of whatever the
// cache holds behind a run, reaches the MFMAs.
struct SegWalk {
  int a0, a1, b0, b1;
};

template <bool kPartial = false, bool kGrouped = false, bool kSeg = false>
__device__ __forceinline__ void attn_kv8_tile(const AttnKv8Args& A, const int head, const int tile, unsigned char* smem, float* part = nullptr,
                                              const GroupWalk W = GroupWalk{}, const GroupStart S0 = GroupStart{}, const SegWalk G = SegWalk{}) {
  static_assert(!(kSeg && (kPartial || kGrouped)), "the two-segment walk is the flat, unsplit launch's");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kvh = head / A.group;
  const int n = lane & 31, h = lane >> 5;
  const int qrow = tile * kRows + wave * 32 + n;
  const bool qok = qrow < A.q_rows;
  const int nta = kSeg ? (G.a1 - G.a0 + kKeys - 1) / kKeys : 0;      // tiles of the first run; the second starts at slot b0 = bofs + 64 nta
  const int bofs = kSeg ? G.b0 - nta * kKeys : 0;
  const int nt = kSeg ? nta + (G.b1 - G.b0 + kKeys - 1) / kKeys : kGrouped ? W.nt : (A.kv_len - A.kv_start + kKeys - 1) / kKeys;
  // grouped walk: the loader's cursor (tile lj of the group that ends at lnext starts at slot lrow) and the compute loop's (tile cj
  // starts at slot crow; its group ends at cnext and has the scale vs; vsp: the group's entry of the scale table)
  int lj = 0, lrow = 0, lnext = W.tokens;
  int cj = 0, crow = 0, cnext = W.tokens;
  const_f32_ptr vsp = (const_f32_ptr)(unsigned long long)(A.v_scale + kvh);
  if constexpr (kPartial && kGrouped) {
    lj = cj = S0.j, lrow = crow = S0.row, lnext = cnext = (S0.g + 1) * W.tokens;
    vsp += S0.g * W.kv_heads;
  }
  float vs = kGrouped ? *vsp : 0.f;

  // ---- q fragments: bytes [64 c + 32 h, +32) of the row, once
  v8i qf[2];
  {
    const unsigned char* qp = A.q + (size_t)(qok ? qrow : 0) * A.ldq + head * 128 + h * 32;
    const v4i z = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const v4i lo = *reinterpret_cast<const v4i*>(qp + c * 64), hi = *reinterpret_cast<const v4i*>(qp + c * 64 + 16);
      qf[c] = cat(qok ? lo : z, qok ? hi : z);
    }
  }

  // ---- loaders.  Rows past kv_len read zeros through the descriptors' bound (the last valid row ends at nrec).
  const unsigned nrec = kSeg ? (G.a1 > G.a0 ? (unsigned)(G.a1 - 1) * (unsigned)A.pitch + 128u : 0u) : (unsigned)(A.kv_len - 1) * (unsigned)A.pitch + 128u;
  const v4i krs = make_rsrc(A.k + kvh * 128, nrec);
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(A.v + kvh * 128), 0, (int)nrec, 0x00020000);
  // kSeg: the second run's descriptors (its own end), and a tile's base slot
  const unsigned nrec_b = kSeg && G.b1 > G.b0 ? (unsigned)(G.b1 - 1) * (unsigned)A.pitch + 128u : 0u;
  const v4i krs_b = kSeg ? make_rsrc(A.k + kvh * 128, nrec_b) : krs;
  const __amdgpu_buffer_rsrc_t vrs_b = kSeg ? __builtin_amdgcn_make_buffer_rsrc((void*)(A.v + kvh * 128), 0, (int)nrec_b, 0x00020000) : vrs;
  auto seg_row = [&](int t) __attribute__((always_inline)) { return (t < nta ? G.a0 : bofs) + t * kKeys; };
  const unsigned lds0 = (unsigned)(unsigned long long)(lds_ptr_t)smem;
  // K: wave w moves rows 8 w + (lane >> 3) of the tile; physical chunk lane & 7 holds logical chunk (lane & 7) ^ ((row >> 1) & 7)
  const int prow = wave * 8 + (lane >> 3);
  const int k_voff = prow * A.pitch + (((lane & 7) ^ ((prow >> 1) & 7)) << 4);
  auto dma_k = [&](int t, int slot) __attribute__((always_inline)) {
    if constexpr (kSeg) dma16(t < nta ? krs : krs_b, lds0 + slot * kSlot + wave * 1024, k_voff, seg_row(t) * A.pitch);
    else dma16(krs, lds0 + slot * kSlot + wave * 1024, k_voff, (kGrouped ? lrow : A.kv_start + t * kKeys) * A.pitch);
  };
  // V: thread (vc, kq) owns channels 4 vc .. 4 vc + 3 of keys 4 kq .. 4 kq + 3
  const int vc = tid & 31, kq = tid >> 5;
  const int v_voff = 4 * kq * A.pitch + 4 * vc;
  unsigned vw[4];
  auto load_v = [&](int t) __attribute__((always_inline)) {
    if constexpr (kSeg) {
      const __amdgpu_buffer_rsrc_t rs = t < nta ? vrs : vrs_b;
#pragma unroll
      for (int j = 0; j < 4; ++j) vw[j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_raw_buffer_load_b32(rs, v_voff + j * A.pitch, seg_row(t) * A.pitch, 0));
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      vw[j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_raw_buffer_load_b32(vrs, v_voff + j * A.pitch, (kGrouped ? lrow : A.kv_start + t * kKeys) * A.pitch, 0));
    if constexpr (kGrouped) {                       // (a tile's V load follows its K DMA: the loader's cursor moves here)
      if (++lj == W.tpg) lj = 0, lrow = lnext, lnext += W.tokens;
      else lrow += kKeys;
    }
  };
  // key quad kq = 8 kb + 2 g + h  ->  bytes [32 h + 16 kb + 4 g, +4) of a V^T row; row d sits at 64 d + 16 (d >> 2)
  const int vt_woff = kKTile + (4 * vc) * 64 + vc * 16 + (kq & 1) * 32 + (kq >> 3) * 16 + ((kq & 7) >> 1) * 4;
  auto store_vt = [&](int slot) __attribute__((always_inline)) {
    const unsigned a = __builtin_amdgcn_perm(vw[1], vw[0], 0x05010400), b = __builtin_amdgcn_perm(vw[1], vw[0], 0x07030602);
    const unsigned c = __builtin_amdgcn_perm(vw[3], vw[2], 0x05010400), d = __builtin_amdgcn_perm(vw[3], vw[2], 0x07030602);
    unsigned char* p = smem + slot * kSlot + vt_woff;
    *reinterpret_cast<unsigned*>(p) = __builtin_amdgcn_perm(c, a, 0x05040100);
    *reinterpret_cast<unsigned*>(p + 64) = __builtin_amdgcn_perm(c, a, 0x07060302);
    *reinterpret_cast<unsigned*>(p + 128) = __builtin_amdgcn_perm(d, b, 0x05040100);
    *reinterpret_cast<unsigned*>(p + 192) = __builtin_amdgcn_perm(d, b, 0x07060302);
  };

  // ---- readers
  const int phase = (n >> 1) & 7;
  int k_roff[2][2];      // [c][part]: 16-byte chunk 4 c + 2 h + part of row n (a 32-key block adds 4096)
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int part = 0; part < 2; ++part) k_roff[c][part] = n * 128 + (((4 * c + 2 * h + part) ^ phase) << 4);
  const int vt_roff = kKTile + n * 64 + (n >> 2) * 16 + h * 32;      // a 32-channel block adds 32 * 64 + 8 * 16

  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = splat16(0.f);
  float m = 0.f, lsum = 0.f;

  dma_k(0, 0);
  load_v(0);
  if (nt > 1) dma_k(1, 1);
  store_vt(0);
  if (nt > 1) load_v(1);

  int slot = 0;
  for (int t = 0; t < nt; ++t) {
    const int slot1 = slot == kRing - 1 ? 0 : slot + 1, slot2 = slot1 == kRing - 1 ? 0 : slot1 + 1;
    wait_vm<0>();                                   // K of tile t (and t + 1) has landed; V of t + 1 is in vw
    if (t + 1 < nt) store_vt(slot1);                // slot1 was last read in iteration t - 2: every wave is past barrier t - 1
    __syncthreads();
    if (t + 2 < nt) {                               // slot2 was last read in iteration t - 1: every wave is past this barrier
      dma_k(t + 2, slot2);
      load_v(t + 2);
    }
    const unsigned char* ks = smem + slot * kSlot;

    // ---- S^T + (7 - m)
    f32x16 s[2];
    const f32x16 cinit = splat16(7.f - m);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const v8i a = cat(*reinterpret_cast<const v4i*>(ks + kb * 4096 + k_roff[c][0]), *reinterpret_cast<const v4i*>(ks + kb * 4096 + k_roff[c][1]));
        s[kb] = mfma8(a, qf[c], c == 0 ? cinit : s[kb]);
      }
    }
    // grouped: keys left in the tile's group (clipped to kv_len); fewer than 64 in a group's last tile, wave-uniformly
    const int gleft = kSeg ? (t < nta ? G.a1 : G.b1) - seg_row(t) : (cnext < A.kv_len ? cnext : A.kv_len) - crow;
    if ((kGrouped || kSeg) ? (gleft < kKeys) : (t == nt - 1)) {   // keys past kv_len (zero K rows, or whatever the cache holds there)
      const int left = (kGrouped || kSeg) ? gleft : A.kv_len - A.kv_start - t * kKeys;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (kb * 32 + (i >> 2) * 8 + h * 4 + (i & 3) >= left) s[kb][i] = -INFINITY;
    }
    float tmax = s[0][0];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, s[kb][i]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const bool first = t == 0;
    if (first || __builtin_amdgcn_ballot_w64(tmax > 8.75f) != 0) {      // wave-uniform
      const float delta = first ? tmax - 7.f : fmaxf(tmax - 7.f, 0.f);
      const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);
      m += delta;
      lsum *= alpha;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[kb][i] -= delta;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
    }

    // ---- P: exp2 -> e4m3, packed in place as the B operand; the row sum from the unrounded values
    v8i pb;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float p0 = __builtin_amdgcn_exp2f(s[kb][4 * g]), p1 = __builtin_amdgcn_exp2f(s[kb][4 * g + 1]);
        const float p2 = __builtin_amdgcn_exp2f(s[kb][4 * g + 2]), p3 = __builtin_amdgcn_exp2f(s[kb][4 * g + 3]);
        lsum += (p0 + p1) + (p2 + p3);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(p2, p3, w, true);
        pb[kb * 4 + g] = w;
      }
    }

    // ---- O^T += V^T P^T
    if constexpr (kGrouped) {
      if (cj == 0 && t > 0) {                       // a new group: O into units of its scale
        const float nv = *vsp;
        if (nv != vs) {
          const float r = vs / nv;
#pragma unroll
          for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) o[db][i] *= r;
          vs = nv;
        }
      }
      if (++cj == W.tpg) cj = 0, crow = cnext, cnext += W.tokens, vsp += W.kv_heads;
      else crow += kKeys;
    }
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const unsigned char* vp = ks + vt_roff + db * (32 * 64 + 8 * 16);
      o[db] = mfma8(cat(*reinterpret_cast<const v4i*>(vp), *reinterpret_cast<const v4i*>(vp + 16)), pb, o[db]);
    }
    slot = slot1;
  }

  // ---- epilogue: lane (n, h) holds channels 32 db + 8 g + 4 h + e of query row n
  const float ltot = lsum + __shfl_xor(lsum, 32);
  if constexpr (kPartial) {
    if (qok) {
      float* pw = part + (size_t)(tile * 8 + wave) * kPartWave;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(pw + (4 * db + g) * 256 + lane * 4) = f32x4{o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]};
      if (h == 0) *reinterpret_cast<f32x4*>(pw + 4096 + n * 4) = f32x4{m, ltot, 0.f, 0.f};
    }
    return;
  }
  if (!qok) return;
  const float f = (kGrouped ? vs : A.v_scale[kvh]) / ltot;      // (the 2^7 of P is in O and in the sum alike; grouped: the last group's scale)
  unsigned short* op = A.out + (size_t)qrow * A.ldo + head * 128 + h * 4;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u16x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = f2bf(o[db][4 * g + e] * f);
      *reinterpret_cast<u16x4*>(op + db * 32 + g * 8) = r;
    }
  if (A.lse != nullptr && h == 0) A.lse[(size_t)head * A.q_rows + qrow] = (m - 7.f + log2f(ltot)) * 0.6931471805599453f;
}

__global__ __launch_bounds__(512) void attn_fwd_kv8_kernel(AttnKv8Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int item = (blockIdx.x & 7) * A.per_xcd + (blockIdx.x >> 3);
  if (item >= A.total) return;
  const int head = item / A.row_tiles;
  attn_kv8_tile(A, head, item - head * A.row_tiles, smem);
}

// The grouped launch (include/inferix_hip_kv8_ring.h): the single launch's raster, the per-group walk along the keys.
struct AttnKv8GroupedArgs {
  AttnKv8Args a;               // kv_start = 0; v_scale is the table [group][kv_head]
  GroupWalk w;
};

__global__ __launch_bounds__(512) void attn_fwd_kv8_grouped_kernel(AttnKv8GroupedArgs G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int item = (blockIdx.x & 7) * G.a.per_xcd + (blockIdx.x >> 3);
  if (item >= G.a.total) return;
  const int head = item / G.a.row_tiles;
  attn_kv8_tile<false, true>(G.a, head, item - head * G.a.row_tiles, smem, nullptr, G.w);
}

// The multi launch (ifx_attn_kv8_multi.h).  Workgroup b is local tile b >> 3 of XCD b & 7; the stream that owns it is the last of
// the XCD's list whose raster word does not exceed the tile: a binary search over kernel arguments, all of it scalar.  What follows
// is the item's own single launch: its AttnKv8Args, so the descriptor bound that zeroes K / V rows past kv_len is this item's.
__global__ __launch_bounds__(512) void attn_fwd_kv8_multi_kernel(AttnKv8MultiArgs T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int x = blockIdx.x & 7, lt = blockIdx.x >> 3;
  if (lt >= T.xcd_tiles[x]) return;
  int lo = T.xcd_first[x], hi = T.xcd_first[x + 1] - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)(T.stream[mid] >> kTile0Shift) <= lt) lo = mid;
    else hi = mid - 1;
  }
  const unsigned w = __builtin_amdgcn_readfirstlane(T.stream[lo]);
  const AttnKv8Item& it = T.item[w & (kMultiItems - 1)];
  const AttnKv8Args A{it.q, it.ldq, it.out, it.ldo, nullptr, it.k, it.v, it.v_scale, it.q_rows, T.group, T.pitch, it.kv_start, it.kv_len,
                      it.row_tiles, 0, 0};
  attn_kv8_tile(A, (int)(w >> kItemBits) & ((1 << kHeadBits) - 1), lt - (int)(w >> kTile0Shift), smem);
}

// The ranges launch (ifx_attn_kv8_multi.h, include/inferix_hip_kv8_magi.h): the multi launch's scalar prologue over streams that are
// (range, kv head) pairs.  A stream's local tiles are its `group` query heads x the range's row tiles, head-major, so every workgroup
// that reads a (range, kv head)'s K / V bytes sits on one XCD.  The range's rows are addressed from ITS first row — a row tile never
// holds rows of two ranges — and its keys are the two runs of the cut walk (attn_kv8_tile's kSeg form).
__global__ __launch_bounds__(512) void attn_fwd_kv8_ranges_kernel(AttnKv8RangesArgs T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int x = blockIdx.x & 7, lt = blockIdx.x >> 3;
  if (lt >= T.xcd_tiles[x]) return;
  int lo = T.xcd_first[x], hi = T.xcd_first[x + 1] - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)(T.stream[mid] >> kTile0Shift) <= lt) lo = mid;
    else hi = mid - 1;
  }
  const unsigned w = __builtin_amdgcn_readfirstlane(T.stream[lo]);
  const AttnKv8Range& r = T.range[w & (kRanges - 1)];
  const int local = lt - (int)(w >> kTile0Shift);
  const int hg = local / r.row_tiles;
  const int head = ((int)(w >> kItemBits) & ((1 << kHeadBits) - 1)) * T.group + hg;
  const AttnKv8Args A{T.q + (size_t)r.q0 * T.ldq, T.ldq, T.out + (size_t)r.q0 * T.ldo, T.ldo, nullptr, T.k, T.v, T.v_scale, r.q_rows, T.group, T.pitch,
                      0, 0, r.row_tiles, 0, 0};
  attn_kv8_tile<false, false, true>(A, head, local - hg * r.row_tiles, smem, nullptr, GroupWalk{}, GroupStart{}, SegWalk{r.a0, r.a1, r.b0, r.b1});
}

// The split-key launch (ifx_attn_kv8.h, include/inferix_hip_kv8_split.h).  Workgroup b is local item b >> 3 of XCD b & 7: chunk
// (b >> 3) % chunks of that XCD's group (b >> 3) / chunks, a group being a (head, row tile) of the single launch.  The workgroup runs
// the single launch's loop over its chunk's keys (a whole number of 64-key tiles from kv_start; the descriptor bound that zeroes K / V
// rows past the end is the chunk's end) and leaves fp32 partials.  Then: device-scope release, ONE atomic add on the group's arrival
// counter; whoever reads chunks - 1 is last, acquires, and merges every chunk's rows — its own included, from the workspace — in chunk
// order.  Nobody waits for anybody.  The counters are zeroed on the stream ahead of this kernel (kv8_split_clear_kernel).
struct AttnKv8SplitArgs {
  AttnKv8Args a;               // the launch as a whole: kv_start / kv_len are the full key range
  float* part;                 // [chunks][heads][row_tiles][8 waves][kPartWave]
  int* arrived;                // [row_tiles * heads]
  int heads, chunks, tiles_lo, tiles_rem;      // chunk c holds tiles_lo + (c < tiles_rem) key tiles
  int xcd_first[9];            // groups [xcd_first[x], xcd_first[x + 1]) are XCD x's
};

__global__ __launch_bounds__(256) void kv8_split_clear_kernel(int* arrived, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) arrived[i] = 0;
}

__global__ __launch_bounds__(512) void attn_fwd_kv8_split_kernel(AttnKv8SplitArgs S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int x = blockIdx.x & 7, li = blockIdx.x >> 3;
  const int lg = li / S.chunks, chunk = li - lg * S.chunks;
  if (lg >= S.xcd_first[x + 1] - S.xcd_first[x]) return;
  const int group = S.xcd_first[x] + lg;
  const int head = group / S.a.row_tiles, tile = group - head * S.a.row_tiles;
  const int t0 = chunk * S.tiles_lo + min(chunk, S.tiles_rem), t1 = t0 + S.tiles_lo + (chunk < S.tiles_rem ? 1 : 0);
  AttnKv8Args A = S.a;
  A.kv_start = S.a.kv_start + t0 * kKeys;
  A.kv_len = min(S.a.kv_len, S.a.kv_start + t1 * kKeys);
  const size_t head_words = (size_t)S.a.row_tiles * 8 * kPartWave, chunk_words = head_words * S.heads;
  attn_kv8_tile<true>(A, head, tile, smem, S.part + chunk * chunk_words + head * head_words);

  // ---- arrival.  Every thread's partial stores are released to the device before the barrier; the one atomic follows it.
  __threadfence();
  __syncthreads();                                  // (and: every wave is past its last LDS read)
  int* last = reinterpret_cast<int*>(smem);
  if (threadIdx.x == 0) *last = __hip_atomic_fetch_add(S.arrived + group, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S.chunks - 1;
  __syncthreads();
  if (*last == 0) return;
  __threadfence();                                  // acquire: the other chunks' partials, whichever XCD wrote them

  // ---- merge, in chunk order: wave w rows 32 w .. 32 w + 31 of the tile, lane (n, h) the 16-byte pieces it wrote in the main loop
  const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
  const int qrow = tile * kRows + (threadIdx.x >> 6) * 32 + n;
  if (qrow >= S.a.q_rows) return;
  const float* p0 = S.part + head * head_words + (size_t)(tile * 8 + (threadIdx.x >> 6)) * kPartWave;
  float M = -INFINITY;
  for (int c = 0; c < S.chunks; ++c) M = fmaxf(M, p0[c * chunk_words + 4096 + n * 4]);
  f32x4 acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int c = 0; c < S.chunks; ++c) {
    const float* pc = p0 + c * chunk_words;
    const f32x4 ml = *reinterpret_cast<const f32x4*>(pc + 4096 + n * 4);
    const float w = __builtin_amdgcn_exp2f(ml[0] - M);
    L += w * ml[1];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += w * *reinterpret_cast<const f32x4*>(pc + j * 256 + lane * 4);
  }
  const float f = S.a.v_scale[head / S.a.group] / L;
  unsigned short* op = S.a.out + (size_t)qrow * S.a.ldo + head * 128 + h * 4;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    u16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = f2bf(acc[j][e] * f);
    *reinterpret_cast<u16x4*>(op + (j >> 2) * 32 + (j & 3) * 8) = r;
  }
  if (S.a.lse != nullptr && h == 0) S.a.lse[(size_t)head * S.a.q_rows + qrow] = (M - 7.f + log2f(L)) * 0.6931471805599453f;
}

// The grouped split-key launch (include/inferix_hip_kv8_ring_split.h): attn_fwd_kv8_split_kernel's raster, arrival and merge around
// the grouped walk.  Chunk c is nt[c] tiles of the walk from tile j0[c] of group g0[c] (host arithmetic: the kernel multiplies, it does
// not divide) and leaves O in units of the scale of group glast[c].  The merging workgroup reads those scales from the table — scalar
// loads of memory this launch never writes — and sums in units of the LAST chunk's scale: chunk c weighs w_c s_c / s_last, exact for
// powers of two, and 1 where the scales are equal, which makes the merge attn_fwd_kv8_split_kernel's own operation for operation.
struct AttnKv8GroupedSplitArgs {
  AttnKv8Args a;               // the launch as a whole: kv_start = 0, kv_len the end of the walk, v_scale the table [group][kv_head]
  float* part;                 // [chunks][heads][row_tiles][8 waves][kPartWave]
  int* arrived;                // [row_tiles * heads]
  int heads, chunks, tokens, tpg, kv_heads;
  int xcd_first[9];            // groups [xcd_first[x], xcd_first[x + 1]) are XCD x's
  int nt[kMaxSplits], g0[kMaxSplits], j0[kMaxSplits], glast[kMaxSplits];
};

__global__ __launch_bounds__(512) void attn_fwd_kv8_grouped_split_kernel(AttnKv8GroupedSplitArgs S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int x = blockIdx.x & 7, li = blockIdx.x >> 3;
  const int lg = li / S.chunks, chunk = li - lg * S.chunks;
  if (lg >= S.xcd_first[x + 1] - S.xcd_first[x]) return;
  const int group = S.xcd_first[x] + lg;
  const int head = group / S.a.row_tiles, tile = group - head * S.a.row_tiles;
  const int g0 = S.g0[chunk], j0 = S.j0[chunk];
  const size_t head_words = (size_t)S.a.row_tiles * 8 * kPartWave, chunk_words = head_words * S.heads;
  attn_kv8_tile<true, true>(S.a, head, tile, smem, S.part + chunk * chunk_words + head * head_words,
                            GroupWalk{S.tokens, S.tpg, S.nt[chunk], S.kv_heads}, GroupStart{g0, j0, g0 * S.tokens + j0 * kKeys});

  // ---- arrival, as attn_fwd_kv8_split_kernel: release, barrier, one atomic per workgroup; the last one acquires and merges
  __threadfence();
  __syncthreads();                                  // (and: every wave is past its last LDS read)
  int* last = reinterpret_cast<int*>(smem);
  if (threadIdx.x == 0) *last = __hip_atomic_fetch_add(S.arrived + group, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S.chunks - 1;
  __syncthreads();
  if (*last == 0) return;
  __threadfence();

  // ---- merge, in chunk order, in units of the last chunk's scale
  const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
  const int qrow = tile * kRows + (threadIdx.x >> 6) * 32 + n;
  if (qrow >= S.a.q_rows) return;
  const float* p0 = S.part + head * head_words + (size_t)(tile * 8 + (threadIdx.x >> 6)) * kPartWave;
  const_f32_ptr tab = (const_f32_ptr)(unsigned long long)(S.a.v_scale + head / S.a.group);
  const float s_last = tab[S.glast[S.chunks - 1] * S.kv_heads];
  float M = -INFINITY;
  for (int c = 0; c < S.chunks; ++c) M = fmaxf(M, p0[c * chunk_words + 4096 + n * 4]);
  f32x4 acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float L = 0.f;
  for (int c = 0; c < S.chunks; ++c) {
    const float* pc = p0 + c * chunk_words;
    const f32x4 ml = *reinterpret_cast<const f32x4*>(pc + 4096 + n * 4);
    const float w = __builtin_amdgcn_exp2f(ml[0] - M);
    L += w * ml[1];
    const float ws = w * (tab[S.glast[c] * S.kv_heads] / s_last);
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += ws * *reinterpret_cast<const f32x4*>(pc + j * 256 + lane * 4);
  }
  const float f = s_last / L;
  unsigned short* op = S.a.out + (size_t)qrow * S.a.ldo + head * 128 + h * 4;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    u16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = f2bf(acc[j][e] * f);
    *reinterpret_cast<u16x4*>(op + (j >> 2) * 32 + (j & 3) * 8) = r;
  }
  if (S.a.lse != nullptr && h == 0) S.a.lse[(size_t)head * S.a.q_rows + qrow] = (M - 7.f + log2f(L)) * 0.6931471805599453f;
}

// ---------------------------------------------------------------------------
// One wave per token, as rmsnorm_rope_append_kernel: every load requested up front and branch-free, the (cos, sin) pairs once per token.
// RMS scale -> bf16 -> x weight -> bf16 -> rotation (fp64 -> fp32) -> x out_scale -> e4m3 bytes at dst[0, dim)
template <int NCH>
__device__ __forceinline__ void rmsnorm_rope_row8(Row<NCH>& row, const u16x8 (&raw)[NCH], const u16x8 (&wv)[NCH], const RopeToken& tk,
                                                  const RopeArgs& ra, float out_scale, int dim, int head_dim, float eps, int lane,
                                                  unsigned char* dst) {
  row.from(raw, dim, lane);
  const float rs = 1.0f / sqrtf(wave_sum(row.sumsq()) / (float)dim + eps);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = rbf(rbf(row.v[c][i] * rs) * bf2f(wv[c][i]));
    if (tk.shared_cs) rope4_cs(t, tk.cs4);
    else if (col < dim) rope4(t, (col % head_dim) >> 1, ra, tk.half, tk.n_t, tk.n_h, tk.pos_t, tk.pos_h, tk.pos_w);
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] *= out_scale;
    const u32x2 pk = pack_e4m3(t);
    if (col < dim) *reinterpret_cast<u32x2*>(dst + col) = pk;
  }
}

// Token `r` of one append: the wave's whole work.
template <int NCH>
__device__ __forceinline__ void kv8_append_row(const unsigned short* __restrict__ qkv, int ld, unsigned char* __restrict__ q8,
                                               const unsigned short* __restrict__ wq, const unsigned short* __restrict__ wk,
                                               const RopeArgs& ra, unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                               const float* __restrict__ v_scale, int local_start, int r, int dim, int head_dim, float eps,
                                               int lane) {
  const unsigned short* base = qkv + (size_t)r * ld;
  const size_t slot_off = (size_t)(local_start + r) * dim;
  const RopeToken tk(ra, 1, r, head_dim, lane);
  u16x8 qraw[NCH], kraw[NCH], vraw[NCH], wqv[NCH], wkv[NCH];
  load_chunks<NCH>(qraw, base, dim, lane);
  load_chunks<NCH>(wqv, wq, dim, lane);
  load_chunks<NCH>(kraw, base + dim, dim, lane);
  load_chunks<NCH>(vraw, base + 2 * dim, dim, lane);
  load_chunks<NCH>(wkv, wk, dim, lane);
  // ---- v / v_scale[head]: a lane's 8 channels lie in one head (head_dim % 8 == 0)
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = c * 512 + lane * 8;
    const float sc = v_scale[col < dim ? col / head_dim : 0];
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = bf2f(vraw[c][i]) / sc;
    const u32x2 pk = pack_e4m3(t);
    if (col < dim) *reinterpret_cast<u32x2*>(vc + slot_off + col) = pk;
  }
  Row<NCH> row;
  rmsnorm_rope_row8<NCH>(row, qraw, wqv, tk, ra, ra.q_scale, dim, head_dim, eps, lane, q8 + (size_t)r * dim);
  rmsnorm_rope_row8<NCH>(row, kraw, wkv, tk, ra, 1.0f, dim, head_dim, eps, lane, kc + slot_off);
}

template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_rope_kv8_append_kernel(const unsigned short* __restrict__ qkv, int ld,
                                                                      unsigned char* __restrict__ q8, const unsigned short* __restrict__ wq,
                                                                      const unsigned short* __restrict__ wk, RopeArgs ra,
                                                                      unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                                      const float* __restrict__ v_scale, int local_start, int rows, int dim,
                                                                      int head_dim, float eps) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  kv8_append_row<NCH>(qkv, ld, q8, wq, wk, ra, kc, vc, v_scale, local_start, r, dim, head_dim, eps, threadIdx.x & 63);
}

// The rows of up to 8 appends in one launch: wave (4 b + w) is row `gr` of the concatenated rows; its item is found from the
// by-value prefix row0, wave-uniformly, and the row is that item's own.
template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_rope_kv8_append_multi_kernel(Kv8AppendMultiArgs T) {
  const int gr = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (gr >= T.row0[kMultiItems]) return;
  int i = 0;
#pragma unroll
  for (int j = 1; j < kMultiItems; ++j)
    if (gr >= T.row0[j]) i = j;
  const Kv8AppendItem& it = T.item[i];
  kv8_append_row<NCH>(it.qkv, it.ld, it.q8, T.wq, T.wk, it.ra, it.k, it.v, it.v_scale, it.local_start, gr - T.row0[i], T.dim, T.head_dim,
                      T.eps, threadIdx.x & 63);
}

// The append into a ring cache (include/inferix_hip_kv8_ring.h).  The wave's token has ONE slot and ONE row of the scale table: both
// are found in scalar code, then the row is kv8_append_row's with that slot and that scale row.  `start` arrives reduced by the host
// (start - ring_base < ring_len where start >= ring_base) and rows <= ring_len, so the wrap is one conditional subtraction.
struct Kv8RingArgs {
  int ring_base, ring_len, start, group_tokens, kv_heads;
};

template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_rope_kv8_append_ring_kernel(const unsigned short* __restrict__ qkv, int ld,
                                                                           unsigned char* __restrict__ q8, const unsigned short* __restrict__ wq,
                                                                           const unsigned short* __restrict__ wk, RopeArgs ra,
                                                                           unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                                           const float* __restrict__ v_scale, Kv8RingArgs R, int rows, int dim,
                                                                           int head_dim, float eps) {
  const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (r >= rows) return;
  int slot = R.start + r;
  if (slot >= R.ring_base + R.ring_len) slot -= R.ring_len;
  const int grp = (int)((unsigned)slot / (unsigned)R.group_tokens);
  // (kv8_append_row addresses slot local_start + r and scale v_scale[head])
  kv8_append_row<NCH>(qkv, ld, q8, wq, wk, ra, kc, vc, v_scale + (size_t)grp * R.kv_heads, slot - r, r, dim, head_dim, eps, threadIdx.x & 63);
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_ring_sessions.h
// The grouped launch behind the multi launch's raster: attn_fwd_kv8_multi_kernel's scalar prologue, then the item's own grouped launch
// — its AttnKv8Args and its GroupWalk (the tiles of ITS walk; group size and table row length are the launch's).
__global__ __launch_bounds__(512) void attn_fwd_kv8_grouped_multi_kernel(AttnKv8GroupedMultiArgs T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int x = blockIdx.x & 7, lt = blockIdx.x >> 3;
  if (lt >= T.xcd_tiles[x]) return;
  int lo = T.xcd_first[x], hi = T.xcd_first[x + 1] - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)(T.stream[mid] >> kTile0Shift) <= lt) lo = mid;
    else hi = mid - 1;
  }
  const unsigned w = __builtin_amdgcn_readfirstlane(T.stream[lo]);
  const AttnKv8GroupedItem& it = T.item[w & (kMultiItems - 1)];
  const AttnKv8Args A{it.q, it.ldq, it.out, it.ldo, nullptr, it.k, it.v, it.v_scale, it.q_rows, T.group, T.pitch, 0, it.kv_len, it.row_tiles, 0, 0};
  attn_kv8_tile<false, true>(A, (int)(w >> kItemBits) & ((1 << kHeadBits) - 1), lt - (int)(w >> kTile0Shift), smem, nullptr,
                             GroupWalk{T.tokens, T.tpg, it.nt, T.kv_heads});
}

// The V scale of a frame from its amax (>= 0), in bits: the smallest power of two s with a = max(amax, 2^-20) <= 448 s.  With
// a = m 2^e, 1 <= m < 2, and 448 = 1.75 * 2^8 that is 2^(e - 8) when m <= 1.75 and 2^(e - 7) otherwise; e >= -20 keeps it normal.
__device__ __forceinline__ float kv8_frame_scale(float amax) {
  const unsigned a = __builtin_bit_cast(unsigned, fmaxf(amax, 9.5367431640625e-07f));
  return __builtin_bit_cast(float, ((a >> 23) - 8u + ((a & 0x7fffffu) > 0x600000u ? 1u : 0u)) << 23);
}

// Token `r` of one append into a ring, q and K only: kv8_append_row without the V columns.
template <int NCH>
__device__ __forceinline__ void kv8_append_row_qk(const unsigned short* __restrict__ qkv, int ld, unsigned char* __restrict__ q8,
                                                  const unsigned short* __restrict__ wq, const unsigned short* __restrict__ wk,
                                                  const RopeArgs& ra, unsigned char* __restrict__ kdst, int r, int dim, int head_dim, float eps,
                                                  int lane) {
  const unsigned short* base = qkv + (size_t)r * ld;
  const RopeToken tk(ra, 1, r, head_dim, lane);
  u16x8 qraw[NCH], kraw[NCH], wqv[NCH], wkv[NCH];
  load_chunks<NCH>(qraw, base, dim, lane);
  load_chunks<NCH>(wqv, wq, dim, lane);
  load_chunks<NCH>(kraw, base + dim, dim, lane);
  load_chunks<NCH>(wkv, wk, dim, lane);
  Row<NCH> row;
  rmsnorm_rope_row8<NCH>(row, qraw, wqv, tk, ra, ra.q_scale, dim, head_dim, eps, lane, q8 + (size_t)r * dim);
  rmsnorm_rope_row8<NCH>(row, kraw, wkv, tk, ra, 1.0f, dim, head_dim, eps, lane, kdst);
}

// The appends of up to 8 samples into their ring caches WITH the calibration of the frames written, one launch, two kinds of
// workgroup (256 threads either way), none waiting for another:
//   * blocks [0, slab0[8]) — SLAB workgroups, one per (item, frame, kv head), the lowest indices so that they start first.  A frame's
//     V slab is G rows x 128 bf16 of qkv: 256 bytes per row, 16 lanes x 16 bytes, so a wave instruction covers 4 rows and the
//     workgroup 16; kSlabDepth such steps are requested before the first is used (128 rows, 32 KiB in flight).  Pass 1: |v| -> amax
//     over lanes (DPP), waves (LDS).  The scale goes to v_scale[group][head] by thread 0 — an ordinary store — and every thread
//     derives the same value for itself.  Pass 2 reads the slab again (L2: at G = 1560 it is 400 KB) and stores the bytes of
//     kv8_append_row, bf2f(v) / sc through pack_e4m3, to the frame's slots.  Rows past G re-read row G - 1 (pass 1: the amax does not
//     mind) and are not stored.
//   * the rest — ROW workgroups, one wave per token of the concatenated rows: q and K of kv8_append_row, the item from the by-value
//     prefix, the ring slot by one conditional subtraction.  They touch neither V nor the scale table.
// start, ring_base, ring_len and rows are multiples of G (the launcher's check), so a frame of an item is one group of slots.
constexpr int kSlabDepth = 8;

template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_rope_kv8_append_ring_multi_kernel(Kv8RingAppendMultiArgs T) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nslab = T.slab0[kMultiItems];
  if ((int)blockIdx.x >= nslab) {
    const int gr = ((int)blockIdx.x - nslab) * 4 + wave;
    if (gr >= T.row0[kMultiItems]) return;
    int i = 0;
#pragma unroll
    for (int j = 1; j < kMultiItems; ++j)
      if (gr >= T.row0[j]) i = j;
    const Kv8RingAppendItem& it = T.item[i];
    const int r = gr - T.row0[i];
    int slot = it.start + r;
    if (slot >= it.ring_base + it.ring_len) slot -= it.ring_len;
    kv8_append_row_qk<NCH>(it.qkv, it.ld, it.q8, T.wq, T.wk, it.ra, it.k + (size_t)slot * T.dim, r, T.dim, T.head_dim, T.eps, lane);
    return;
  }
  __shared__ float wave_amax[4];
  int i = 0;
#pragma unroll
  for (int j = 1; j < kMultiItems; ++j)
    if ((int)blockIdx.x >= T.slab0[j]) i = j;
  const Kv8RingAppendItem& it = T.item[i];
  const int local = (int)blockIdx.x - T.slab0[i];
  const int frame = local / T.kv_heads, head = local - frame * T.kv_heads;
  const int G = T.group_tokens;
  int slot0 = it.start + frame * G;
  if (slot0 >= it.ring_base + it.ring_len) slot0 -= it.ring_len;
  // lane (lr, lc): row 4 wave + lr of a 16-row step, bytes [16 lc, +16) of the head's 256
  const int lr = lane >> 4, lc = lane & 15;
  const unsigned short* src = it.qkv + (size_t)frame * G * it.ld + 2 * T.dim + head * 128 + lc * 8;
  const int row_in_step = wave * 4 + lr;
  float amax = 0.f;
  for (int r0 = 0; r0 < G; r0 += 16 * kSlabDepth) {
    u16x8 u[kSlabDepth];
#pragma unroll
    for (int d = 0; d < kSlabDepth; ++d) {
      const int r = r0 + d * 16 + row_in_step;
      u[d] = *reinterpret_cast<const u16x8*>(src + (size_t)(r < G ? r : G - 1) * it.ld);
    }
#pragma unroll
    for (int d = 0; d < kSlabDepth; ++d)
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(u[d][e])));
  }
  amax = wave_max(amax);
  if (lane == 0) wave_amax[wave] = amax;
  __syncthreads();
  const float sc = kv8_frame_scale(fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3])));
  if (threadIdx.x == 0) it.v_scale[(size_t)(slot0 / G) * T.kv_heads + head] = sc;
  unsigned char* dst = it.v + (size_t)slot0 * T.dim + head * 128 + lc * 8;
  for (int r0 = 0; r0 < G; r0 += 16 * kSlabDepth) {
    u16x8 u[kSlabDepth];
#pragma unroll
    for (int d = 0; d < kSlabDepth; ++d) {
      const int r = r0 + d * 16 + row_in_step;
      u[d] = *reinterpret_cast<const u16x8*>(src + (size_t)(r < G ? r : G - 1) * it.ld);
    }
#pragma unroll
    for (int d = 0; d < kSlabDepth; ++d) {
      const int r = r0 + d * 16 + row_in_step;
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = bf2f(u[d][e]) / sc;
      const u32x2 pk = pack_e4m3(t);
      if (r < G) *reinterpret_cast<u32x2*>(dst + (size_t)r * T.dim) = pk;
    }
  }
}

}  // namespace
}  // namespace ifx

using namespace ifx;

extern "C" int ifx_attn_kv8_plan(int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, ifx_kv8_plan* plan) {
  IFX_REQUIRE(kv8::plan(q_rows, heads, kv_start, kv_len, plan), "ifx_attn_kv8_plan: bad arguments (rows %d, heads %d, keys [%d, %d))", q_rows,
              heads, kv_start, kv_len);
  return IFX_OK;
}

extern "C" int ifx_rmsnorm_rope_kv8_append(const ifx_bf16* qkv, int32_t ld, uint8_t* q8_out, const ifx_bf16* wq, const ifx_bf16* wk,
                                           const ifx_rope_grid* rope, const ifx_kv8_view* view, int32_t local_start, int32_t rows,
                                           int32_t dim, float eps, void* stream) {
  const char* who = "ifx_rmsnorm_rope_kv8_append";
  IFX_REQUIRE(qkv && q8_out && wq && wk && rope && view && rows >= 0 && dim > 0 && dim % 8 == 0 && ld % 8 == 0, "%s: bad arguments", who);
  IFX_REQUIRE(view->k && view->v && view->v_scale && view->kv_heads > 0 && view->kv_heads * view->head_dim == dim,
              "%s: kv view (heads %d x head_dim %d) does not match dim %d", who, view->kv_heads, view->head_dim, dim);
  IFX_REQUIRE(local_start >= 0 && (long long)local_start + rows <= view->num_slots, "%s: append [%d, %d) exceeds cache capacity %d", who,
              local_start, local_start + rows, view->num_slots);
  IFX_REQUIRE(ld >= 3 * dim, "%s: qkv_row_stride (ld %d) must cover the 3 x dim (%d) columns read", who, ld, dim);
  IFX_REQUIRE(rope->flags == 0, "%s: rope flags %d (the V rows are always taken from qkv)", who, rope->flags);
  IFX_REQUIRE(rope->q_scale >= 0.f && rope->q_scale == rope->q_scale, "%s: q_scale must be >= 0 (0 = 1)", who);
  if (view->head_dim != 128) {
    set_error("%s: head_dim %d (built for 128)", who, view->head_dim);
    return IFX_EUNSUP;
  }
  RopeArgs ra{};
  if (const int rc = resolve_rope(who, rope, view->head_dim, dim, rows, &ra)) return rc;
  ra.q_scale = rope->q_scale > 0.f ? rope->q_scale : 1.0f;
  if (rows == 0) return IFX_OK;
  return dispatch_nch<3, 4, 6>(dim, "ifx_rmsnorm_rope_kv8_append: dim %d is wider than the 3072 channels built", [&](auto nch) {
    return launch_rows(who, rmsnorm_rope_kv8_append_kernel<decltype(nch)::value>, rows, stream, qkv, ld, (unsigned char*)q8_out, wq, wk, ra,
                       (unsigned char*)view->k, (unsigned char*)view->v, view->v_scale, local_start, rows, dim, view->head_dim, eps);
  });
}

// What ifx_attn_fwd_kv8 and ifx_attn_fwd_kv8_split refuse alike; ldq / ldo come back resolved.
static int attn_kv8_check(const char* who, const uint8_t* q8, int32_t& ldq, const ifx_bf16* out, int32_t& ldo, const ifx_kv8_view* view,
                          int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len) {
  IFX_REQUIRE(q8 && out && view && view->k && view->v && view->v_scale && q_rows >= 0 && heads > 0, "%s: bad arguments", who);
  IFX_REQUIRE(view->kv_heads > 0 && heads % view->kv_heads == 0, "%s: heads %d is no multiple of kv_heads %d", who, heads, view->kv_heads);
  IFX_REQUIRE(kv_start >= 0 && kv_len > kv_start && kv_len <= view->num_slots, "%s: keys [%d, %d) outside the cache's %d slots", who, kv_start,
              kv_len, view->num_slots);
  if (ldq == 0) ldq = heads * 128;
  if (ldo == 0) ldo = heads * 128;
  IFX_REQUIRE(ldq >= heads * 128 && ldq % 16 == 0 && ((uintptr_t)q8 & 15) == 0, "%s: q row stride %d (bytes) must be >= heads * 128, q 16-byte aligned", who, ldq);
  IFX_REQUIRE(ldo >= heads * 128 && ldo % 8 == 0 && ((uintptr_t)out & 7) == 0, "%s: out row stride %d must be >= heads * 128 and %% 8", who, ldo);
  const long long pitch = (long long)view->kv_heads * 128;
  if (view->head_dim != 128 || (long long)view->num_slots * pitch >= (1ll << 31)) {
    set_error("%s: head_dim %d / cache of %lld bytes (built for head_dim 128, caches below 2 GiB)", who, view->head_dim, view->num_slots * pitch);
    return IFX_EUNSUP;
  }
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const ifx_kv8_view* view,
                                int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, void* stream) {
  const char* who = "ifx_attn_fwd_kv8";
  if (const int rc = attn_kv8_check(who, q8, ldq, out, ldo, view, q_rows, heads, kv_start, kv_len)) return rc;
  if (q_rows == 0) return IFX_OK;
  ifx_kv8_plan p;
  kv8::plan(q_rows, heads, kv_start, kv_len, &p);
  const AttnKv8Args a{q8, ldq, out, ldo, lse, view->k, view->v, view->v_scale, q_rows, heads / view->kv_heads, view->kv_heads * 128, kv_start,
                      kv_len, p.row_tiles, p.row_tiles * heads, p.per_xcd};
  if (const int rc = launch_lds<attn_fwd_kv8_kernel>(dim3(p.grid), dim3(512), p.lds_bytes, (hipStream_t)stream, who, a)) return rc;
  return check_launch(who);
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_split.h
extern "C" int ifx_attn_kv8_split_plan(int32_t q_rows, int32_t heads, int32_t kv_start, int32_t kv_len, int32_t num_splits,
                                       ifx_kv8_split_plan* plan) {
  IFX_REQUIRE(kv8::split_plan(q_rows, heads, kv_start, kv_len, num_splits, attn_kv8_split_min_tiles(), plan),
              "ifx_attn_kv8_split_plan: bad arguments (rows %d, heads %d, keys [%d, %d), splits %d: 0 .. %d)", q_rows, heads, kv_start, kv_len,
              num_splits, kMaxSplits);
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8_split(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const uint8_t* k, const uint8_t* v,
                                      const float* v_scale, int32_t num_slots, int32_t kv_heads, int32_t q_rows, int32_t heads,
                                      int32_t kv_start, int32_t kv_len, int32_t num_splits, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  const char* who = "ifx_attn_fwd_kv8_split";
  const ifx_kv8_view view{(uint8_t*)k, (uint8_t*)v, v_scale, num_slots, kv_heads, 128};
  if (const int rc = attn_kv8_check(who, q8, ldq, out, ldo, &view, q_rows, heads, kv_start, kv_len)) return rc;
  IFX_REQUIRE(num_splits >= 1 && num_splits <= kMaxSplits, "%s: num_splits %d outside [1, %d]", who, num_splits, kMaxSplits);
  if (q_rows == 0) return IFX_OK;
  ifx_kv8_split_plan p;
  kv8::split_plan(q_rows, heads, kv_start, kv_len, num_splits, 0, &p);
  if (p.chunks == 1) return ifx_attn_fwd_kv8(q8, ldq, out, ldo, lse, &view, q_rows, heads, kv_start, kv_len, stream);
  IFX_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= p.workspace_bytes,
              "%s: %d chunks need a 16-byte aligned workspace of %lld bytes (got %p, %lld bytes)", who, p.chunks, (long long)p.workspace_bytes,
              workspace, (long long)workspace_bytes);
  AttnKv8SplitArgs s{};
  s.a = AttnKv8Args{q8, ldq, out, ldo, lse, k, v, v_scale, q_rows, heads / kv_heads, kv_heads * 128, kv_start, kv_len, p.row_tiles, 0, 0};
  s.arrived = (int*)workspace, s.part = (float*)((char*)workspace + p.counter_bytes);
  s.heads = heads, s.chunks = p.chunks, s.tiles_lo = p.key_tiles / p.chunks, s.tiles_rem = p.key_tiles % p.chunks;
  for (int x = 0; x < 8; ++x) s.xcd_first[x + 1] = s.xcd_first[x] + p.xcd_groups[x];
  const int groups = p.row_tiles * heads;
  hipLaunchKernelGGL(kv8_split_clear_kernel, dim3((groups + 255) / 256), dim3(256), 0, (hipStream_t)stream, s.arrived, groups);
  if (const int rc = launch_lds<attn_fwd_kv8_split_kernel>(dim3(p.grid), dim3(512), p.lds_bytes, (hipStream_t)stream, who, s)) return rc;
  return check_launch(who);
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_ring.h
extern "C" int ifx_attn_kv8_grouped_plan(int32_t q_rows, int32_t heads, int32_t group_tokens, int32_t kv_len, ifx_kv8_grouped_plan* plan) {
  IFX_REQUIRE(kv8::grouped_plan(q_rows, heads, group_tokens, kv_len, plan),
              "ifx_attn_kv8_grouped_plan: bad arguments (rows %d, heads %d, groups of %d, keys [0, %d))", q_rows, heads, group_tokens, kv_len);
  return IFX_OK;
}

static int kv8_ring_view_check(const char* who, const ifx_kv8_ring_view* view) {
  IFX_REQUIRE(view && view->k && view->v && view->v_scale && view->kv_heads > 0 && view->num_slots > 0, "%s: bad cache view", who);
  IFX_REQUIRE(view->group_tokens > 0 && view->num_slots % view->group_tokens == 0, "%s: %d slots are no whole number of groups of %d", who,
              view->num_slots, view->group_tokens);
  return IFX_OK;
}

extern "C" int ifx_rmsnorm_rope_kv8_append_ring(const ifx_bf16* qkv, int32_t ld, uint8_t* q8_out, const ifx_bf16* wq, const ifx_bf16* wk,
                                                const ifx_rope_grid* rope, const ifx_kv8_ring_view* view, int32_t ring_base, int32_t ring_len,
                                                int32_t start, int32_t rows, int32_t dim, float eps, void* stream) {
  const char* who = "ifx_rmsnorm_rope_kv8_append_ring";
  IFX_REQUIRE(qkv && q8_out && wq && wk && rope && view && rows >= 0 && dim > 0 && dim % 8 == 0 && ld % 8 == 0, "%s: bad arguments", who);
  if (const int rc = kv8_ring_view_check(who, view)) return rc;
  IFX_REQUIRE((long long)view->kv_heads * view->head_dim == dim, "%s: kv view (heads %d x head_dim %d) does not match dim %d", who,
              view->kv_heads, view->head_dim, dim);
  IFX_REQUIRE(ring_base >= 0 && ring_len > 0 && (long long)ring_base + ring_len <= view->num_slots,
              "%s: ring [%d, %d + %d) outside the cache's %d slots", who, ring_base, ring_base, ring_len, view->num_slots);
  IFX_REQUIRE(start >= 0 && rows <= ring_len, "%s: %d rows from position %d into a ring of %d slots", who, rows, start, ring_len);
  IFX_REQUIRE(ld >= 3 * dim, "%s: qkv_row_stride (ld %d) must cover the 3 x dim (%d) columns read", who, ld, dim);
  IFX_REQUIRE(rope->flags == 0, "%s: rope flags %d (the V rows are always taken from qkv)", who, rope->flags);
  IFX_REQUIRE(rope->q_scale >= 0.f && rope->q_scale == rope->q_scale, "%s: q_scale must be >= 0 (0 = 1)", who);
  if (view->head_dim != 128) {
    set_error("%s: head_dim %d (built for 128)", who, view->head_dim);
    return IFX_EUNSUP;
  }
  RopeArgs ra{};
  if (const int rc = resolve_rope(who, rope, view->head_dim, dim, rows, &ra)) return rc;
  ra.q_scale = rope->q_scale > 0.f ? rope->q_scale : 1.0f;
  if (rows == 0) return IFX_OK;
  const Kv8RingArgs R{ring_base, ring_len, start < ring_base ? start : ring_base + (start - ring_base) % ring_len, view->group_tokens,
                      view->kv_heads};
  return dispatch_nch<3, 4, 6>(dim, "ifx_rmsnorm_rope_kv8_append_ring: dim %d is wider than the 3072 channels built", [&](auto nch) {
    return launch_rows(who, rmsnorm_rope_kv8_append_ring_kernel<decltype(nch)::value>, rows, stream, qkv, ld, (unsigned char*)q8_out, wq, wk, ra,
                       (unsigned char*)view->k, (unsigned char*)view->v, view->v_scale, R, rows, dim, view->head_dim, eps);
  });
}

extern "C" int ifx_attn_fwd_kv8_grouped(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const ifx_kv8_ring_view* view,
                                        int32_t q_rows, int32_t heads, int32_t kv_len, void* stream) {
  const char* who = "ifx_attn_fwd_kv8_grouped";
  if (const int rc = kv8_ring_view_check(who, view)) return rc;
  const ifx_kv8_view flat{view->k, view->v, view->v_scale, view->num_slots, view->kv_heads, view->head_dim};
  if (const int rc = attn_kv8_check(who, q8, ldq, out, ldo, &flat, q_rows, heads, 0, kv_len)) return rc;
  if (q_rows == 0) return IFX_OK;
  ifx_kv8_grouped_plan p;
  kv8::grouped_plan(q_rows, heads, view->group_tokens, kv_len, &p);
  AttnKv8GroupedArgs g{};
  g.a = AttnKv8Args{q8, ldq, out, ldo, lse, view->k, view->v, view->v_scale, q_rows, heads / view->kv_heads, view->kv_heads * 128, 0, kv_len,
                    p.row_tiles, p.row_tiles * heads, p.per_xcd};
  g.w = GroupWalk{view->group_tokens, p.tiles_per_group, p.key_tiles, view->kv_heads};
  if (const int rc = launch_lds<attn_fwd_kv8_grouped_kernel>(dim3(p.grid), dim3(512), p.lds_bytes, (hipStream_t)stream, who, g)) return rc;
  return check_launch(who);
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_ring_split.h
extern "C" int ifx_attn_kv8_grouped_split_plan(int32_t q_rows, int32_t heads, int32_t group_tokens, int32_t kv_len, int32_t num_splits,
                                               ifx_kv8_grouped_split_plan* plan) {
  IFX_REQUIRE(kv8::grouped_split_plan(q_rows, heads, group_tokens, kv_len, num_splits, attn_kv8_grouped_split_min_tiles(), plan),
              "ifx_attn_kv8_grouped_split_plan: bad arguments (rows %d, heads %d, groups of %d, keys [0, %d), splits %d: 0 .. %d)", q_rows, heads,
              group_tokens, kv_len, num_splits, kMaxSplits);
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8_grouped_split(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, float* lse, const uint8_t* k,
                                              const uint8_t* v, const float* v_scale_table, int32_t num_slots, int32_t kv_heads,
                                              int32_t group_tokens, int32_t q_rows, int32_t heads, int32_t kv_len, int32_t num_splits,
                                              void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "ifx_attn_fwd_kv8_grouped_split";
  const ifx_kv8_ring_view ring{(uint8_t*)k, (uint8_t*)v, v_scale_table, num_slots, kv_heads, 128, group_tokens};
  if (const int rc = kv8_ring_view_check(who, &ring)) return rc;
  const ifx_kv8_view flat{ring.k, ring.v, v_scale_table, num_slots, kv_heads, 128};
  if (const int rc = attn_kv8_check(who, q8, ldq, out, ldo, &flat, q_rows, heads, 0, kv_len)) return rc;
  IFX_REQUIRE(num_splits >= 1 && num_splits <= kMaxSplits, "%s: num_splits %d outside [1, %d]", who, num_splits, kMaxSplits);
  if (q_rows == 0) return IFX_OK;
  ifx_kv8_grouped_split_plan p;
  kv8::grouped_split_plan(q_rows, heads, group_tokens, kv_len, num_splits, 0, &p);
  if (p.chunks == 1) return ifx_attn_fwd_kv8_grouped(q8, ldq, out, ldo, lse, &ring, q_rows, heads, kv_len, stream);
  IFX_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= p.workspace_bytes,
              "%s: %d chunks need a 16-byte aligned workspace of %lld bytes (got %p, %lld bytes)", who, p.chunks, (long long)p.workspace_bytes,
              workspace, (long long)workspace_bytes);
  AttnKv8GroupedSplitArgs s{};
  s.a = AttnKv8Args{q8, ldq, out, ldo, lse, k, v, v_scale_table, q_rows, heads / kv_heads, kv_heads * 128, 0, kv_len, p.row_tiles, 0, 0};
  s.arrived = (int*)workspace, s.part = (float*)((char*)workspace + p.counter_bytes);
  s.heads = heads, s.chunks = p.chunks, s.tokens = group_tokens, s.tpg = p.tiles_per_group, s.kv_heads = kv_heads;
  for (int x = 0; x < 8; ++x) s.xcd_first[x + 1] = s.xcd_first[x] + p.xcd_groups[x];
  for (int c = 0; c < p.chunks; ++c) s.nt[c] = p.tiles_per_chunk[c], s.g0[c] = p.first_group[c], s.j0[c] = p.first_tile[c], s.glast[c] = p.last_group[c];
  const int groups = p.row_tiles * heads;
  hipLaunchKernelGGL(kv8_split_clear_kernel, dim3((groups + 255) / 256), dim3(256), 0, (hipStream_t)stream, s.arrived, groups);
  if (const int rc = launch_lds<attn_fwd_kv8_grouped_split_kernel>(dim3(p.grid), dim3(512), p.lds_bytes, (hipStream_t)stream, who, s)) return rc;
  return check_launch(who);
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_sessions.h
extern "C" int ifx_attn_kv8_multi_plan(const int32_t* q_rows, const int32_t* kv_start, const int32_t* kv_len, int32_t n_items, int32_t heads,
                                       ifx_kv8_multi_plan* plan, int32_t* stream_item, int32_t* stream_head, int32_t* stream_tile0,
                                       int32_t capacity) {
  const char* who = "ifx_attn_kv8_multi_plan";
  IFX_REQUIRE(plan && stream_item && stream_head && stream_tile0, "%s: bad arguments", who);
  kv8::MultiPlan p;
  const int rc = kv8::plan_multi(q_rows, kv_start, kv_len, n_items, heads, p);
  if (rc == IFX_EUNSUP) set_error("%s: %d items x %d heads do not fit the raster table (%d streams, %d row tiles per XCD)", who, n_items, heads, kMultiStreams, kMaxTile0);
  IFX_REQUIRE(rc != IFX_EINVAL, "%s: bad arguments (1..%d items, heads > 0, rows >= 0, keys [start, len) not empty)", who, kMultiItems);
  if (rc) return rc;
  IFX_REQUIRE(capacity >= p.n_streams, "%s: %d streams, room for %d", who, p.n_streams, capacity);
  *plan = ifx_kv8_multi_plan{};
  plan->n_streams = p.n_streams, plan->grid = p.grid, plan->lds_bytes = kLds, plan->arg_bytes = (int)sizeof(AttnKv8MultiArgs);
  for (int i = 0; i < n_items; ++i) plan->order[i] = p.order[i];
  for (int x = 0; x < kXcds; ++x) plan->xcd_first[x] = p.xcd_first[x], plan->xcd_tiles[x] = p.xcd_tiles[x], plan->xcd_cost[x] = p.xcd_cost[x];
  plan->xcd_first[kXcds] = p.xcd_first[kXcds];
  for (int s = 0; s < p.n_streams; ++s) stream_item[s] = p.order[p.item[s]], stream_head[s] = p.head[s], stream_tile0[s] = p.tile0[s];
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8_multi(const ifx_attn_kv8_item* items, int32_t n_items, int32_t heads, int32_t kv_heads, void* stream) {
  const char* who = "ifx_attn_fwd_kv8_multi";
  IFX_REQUIRE(items && n_items >= 1 && n_items <= kMultiItems, "%s: 1..%d items per launch (got %d)", who, kMultiItems, n_items);
  IFX_REQUIRE(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, "%s: heads %d is no multiple of kv_heads %d", who, heads, kv_heads);
  const long long pitch = (long long)kv_heads * 128;
  int q_rows[kMultiItems], kv_start[kMultiItems], kv_len[kMultiItems], ldq[kMultiItems], ldo[kMultiItems];
  bool big = false;
  for (int i = 0; i < n_items; ++i) {
    const ifx_attn_kv8_item& it = items[i];
    IFX_REQUIRE(it.q8 && it.out && it.k && it.v && it.v_scale && it.q_rows >= 0, "%s: item %d: bad arguments", who, i);
    IFX_REQUIRE(it.kv_start >= 0 && it.kv_len > it.kv_start && it.kv_len <= it.num_slots, "%s: item %d: keys [%d, %d) outside the cache's %d slots",
                who, i, it.kv_start, it.kv_len, it.num_slots);
    ldq[i] = it.ldq ? it.ldq : heads * 128, ldo[i] = it.ldo ? it.ldo : heads * 128;
    IFX_REQUIRE(ldq[i] >= heads * 128 && ldq[i] % 16 == 0 && ((uintptr_t)it.q8 & 15) == 0,
                "%s: item %d: q row stride %d (bytes) must be >= heads * 128, q 16-byte aligned", who, i, ldq[i]);
    IFX_REQUIRE(ldo[i] >= heads * 128 && ldo[i] % 8 == 0 && ((uintptr_t)it.out & 7) == 0, "%s: item %d: out row stride %d must be >= heads * 128 and %% 8",
                who, i, ldo[i]);
    big = big || (long long)it.num_slots * pitch >= (1ll << 31);
    q_rows[i] = it.q_rows, kv_start[i] = it.kv_start, kv_len[i] = it.kv_len;
  }
  if (big) {
    set_error("%s: a cache of 2 GiB or more (byte offsets are 32-bit)", who);
    return IFX_EUNSUP;
  }
  kv8::MultiPlan p;
  if (kv8::plan_multi(q_rows, kv_start, kv_len, n_items, heads, p) != IFX_OK) {      // (what is IFX_EINVAL there was refused above)
    set_error("%s: %d items x %d heads do not fit the raster table (%d streams, %d row tiles per XCD): launch them one by one", who, n_items,
              heads, kMultiStreams, kMaxTile0);
    return IFX_EUNSUP;
  }
  if (p.n_streams == 0) return IFX_OK;
  AttnKv8MultiArgs a{};
  for (int i = 0; i < n_items; ++i) {
    const int c = p.order[i];
    a.item[i] = AttnKv8Item{items[c].q8, (unsigned short*)items[c].out, items[c].k, items[c].v, items[c].v_scale, ldq[c], ldo[c], q_rows[c],
                            kv_start[c], kv_len[c], (q_rows[c] + kRows - 1) / kRows};
  }
  for (int i = n_items; i < kMultiItems; ++i) a.item[i] = a.item[0];      // never resolved: no raster word names them
  for (int s = 0; s < p.n_streams; ++s) a.stream[s] = (unsigned)p.tile0[s] << kTile0Shift | (unsigned)p.head[s] << kItemBits | (unsigned)p.item[s];
  for (int x = 0; x < kXcds; ++x) a.xcd_first[x] = p.xcd_first[x], a.xcd_tiles[x] = p.xcd_tiles[x];
  a.xcd_first[kXcds] = p.xcd_first[kXcds];
  a.group = heads / kv_heads, a.pitch = (int)pitch;
  if (const int rc = launch_lds<attn_fwd_kv8_multi_kernel>(dim3(p.grid), dim3(512), kLds, (hipStream_t)stream, who, a)) return rc;
  return check_launch(who);
}

extern "C" int ifx_rmsnorm_rope_kv8_append_multi(const ifx_kv8_append_item* items, int32_t n_items, const ifx_bf16* wq, const ifx_bf16* wk,
                                                 int32_t kv_heads, int32_t head_dim, int32_t dim, float eps, void* stream) {
  const char* who = "ifx_rmsnorm_rope_kv8_append_multi";
  IFX_REQUIRE(items && n_items >= 1 && n_items <= kMultiItems, "%s: 1..%d items per launch (got %d)", who, kMultiItems, n_items);
  IFX_REQUIRE(wq && wk && dim > 0 && dim % 8 == 0, "%s: bad arguments", who);
  IFX_REQUIRE(kv_heads > 0 && (long long)kv_heads * head_dim == dim, "%s: kv_heads %d x head_dim %d does not match dim %d", who, kv_heads, head_dim, dim);
  for (int i = 0; i < n_items; ++i) {
    const ifx_kv8_append_item& it = items[i];
    IFX_REQUIRE(it.qkv && it.q8_out && it.rope && it.k && it.v && it.v_scale && it.rows >= 0 && it.qkv_row_stride % 8 == 0, "%s: item %d: bad arguments", who, i);
    IFX_REQUIRE(it.local_start >= 0 && (long long)it.local_start + it.rows <= it.num_slots, "%s: item %d: append [%d, %d) exceeds cache capacity %d",
                who, i, it.local_start, it.local_start + it.rows, it.num_slots);
    IFX_REQUIRE(it.qkv_row_stride >= 3 * dim, "%s: item %d: qkv_row_stride (ld %d) must cover the 3 x dim (%d) columns read", who, i, it.qkv_row_stride, dim);
    IFX_REQUIRE(it.rope->flags == 0, "%s: item %d: rope flags %d (the V rows are always taken from qkv)", who, i, it.rope->flags);
    IFX_REQUIRE(it.rope->q_scale >= 0.f && it.rope->q_scale == it.rope->q_scale, "%s: item %d: q_scale must be >= 0 (0 = 1)", who, i);
  }
  if (head_dim != 128) {
    set_error("%s: head_dim %d (built for 128)", who, head_dim);
    return IFX_EUNSUP;
  }
  Kv8AppendMultiArgs a{};
  for (int i = 0; i < n_items; ++i) {
    const ifx_kv8_append_item& it = items[i];
    Kv8AppendItem& d = a.item[i];
    if (const int rc = resolve_rope(who, it.rope, head_dim, dim, it.rows, &d.ra)) return rc;
    d.ra.q_scale = it.rope->q_scale > 0.f ? it.rope->q_scale : 1.0f;
    d.qkv = it.qkv, d.q8 = it.q8_out, d.k = it.k, d.v = it.v, d.v_scale = it.v_scale, d.ld = it.qkv_row_stride, d.local_start = it.local_start;
    a.row0[i + 1] = a.row0[i] + it.rows;
  }
  for (int i = n_items; i < kMultiItems; ++i) a.item[i] = a.item[0], a.row0[i + 1] = a.row0[n_items];
  a.wq = wq, a.wk = wk, a.n_items = n_items, a.dim = dim, a.head_dim = head_dim, a.eps = eps;
  const int rows = a.row0[kMultiItems];
  if (rows == 0) return IFX_OK;
  return dispatch_nch<3, 4, 6>(dim, "ifx_rmsnorm_rope_kv8_append_multi: dim %d is wider than the 3072 channels built", [&](auto nch) {
    return launch_rows(who, rmsnorm_rope_kv8_append_multi_kernel<decltype(nch)::value>, rows, stream, a);
  });
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_ring_sessions.h
extern "C" int ifx_attn_kv8_grouped_multi_plan(const int32_t* q_rows, const int32_t* kv_len, int32_t n_items, int32_t heads, int32_t group_tokens,
                                               ifx_kv8_grouped_multi_plan* plan, int32_t* stream_item, int32_t* stream_head,
                                               int32_t* stream_tile0, int32_t capacity) {
  const char* who = "ifx_attn_kv8_grouped_multi_plan";
  IFX_REQUIRE(plan && stream_item && stream_head && stream_tile0, "%s: bad arguments", who);
  kv8::MultiPlan p;
  const int rc = kv8::plan_grouped_multi(q_rows, kv_len, n_items, heads, group_tokens, p);
  if (rc == IFX_EUNSUP) set_error("%s: %d items x %d heads do not fit the raster table (%d streams, %d row tiles per XCD)", who, n_items, heads, kMultiStreams, kMaxTile0);
  IFX_REQUIRE(rc != IFX_EINVAL, "%s: bad arguments (1..%d items, heads > 0, groups of > 0 tokens, rows >= 0, keys [0, len) not empty)", who, kMultiItems);
  if (rc) return rc;
  IFX_REQUIRE(capacity >= p.n_streams, "%s: %d streams, room for %d", who, p.n_streams, capacity);
  *plan = ifx_kv8_grouped_multi_plan{};
  plan->n_streams = p.n_streams, plan->grid = p.grid, plan->lds_bytes = kLds, plan->arg_bytes = (int)sizeof(AttnKv8GroupedMultiArgs);
  for (int i = 0; i < n_items; ++i) plan->order[i] = p.order[i];
  for (int x = 0; x < kXcds; ++x) plan->xcd_first[x] = p.xcd_first[x], plan->xcd_tiles[x] = p.xcd_tiles[x], plan->xcd_cost[x] = p.xcd_cost[x];
  plan->xcd_first[kXcds] = p.xcd_first[kXcds];
  for (int s = 0; s < p.n_streams; ++s) stream_item[s] = p.order[p.item[s]], stream_head[s] = p.head[s], stream_tile0[s] = p.tile0[s];
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8_grouped_multi(const ifx_attn_kv8_grouped_item* items, int32_t n_items, int32_t heads, int32_t kv_heads,
                                              int32_t group_tokens, void* stream) {
  const char* who = "ifx_attn_fwd_kv8_grouped_multi";
  IFX_REQUIRE(items && n_items >= 1 && n_items <= kMultiItems, "%s: 1..%d items per launch (got %d)", who, kMultiItems, n_items);
  IFX_REQUIRE(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, "%s: heads %d is no multiple of kv_heads %d", who, heads, kv_heads);
  IFX_REQUIRE(group_tokens > 0, "%s: groups of %d tokens", who, group_tokens);
  const long long pitch = (long long)kv_heads * 128;
  int q_rows[kMultiItems], kv_len[kMultiItems], ldq[kMultiItems], ldo[kMultiItems];
  bool big = false;
  for (int i = 0; i < n_items; ++i) {
    const ifx_attn_kv8_grouped_item& it = items[i];
    IFX_REQUIRE(it.q8 && it.out && it.k && it.v && it.v_scale && it.q_rows >= 0, "%s: item %d: bad arguments", who, i);
    IFX_REQUIRE(it.num_slots > 0 && it.num_slots % group_tokens == 0, "%s: item %d: %d slots are no whole number of groups of %d", who, i,
                it.num_slots, group_tokens);
    IFX_REQUIRE(it.kv_len > 0 && it.kv_len <= it.num_slots, "%s: item %d: keys [0, %d) outside the cache's %d slots", who, i, it.kv_len, it.num_slots);
    ldq[i] = it.ldq ? it.ldq : heads * 128, ldo[i] = it.ldo ? it.ldo : heads * 128;
    IFX_REQUIRE(ldq[i] >= heads * 128 && ldq[i] % 16 == 0 && ((uintptr_t)it.q8 & 15) == 0,
                "%s: item %d: q row stride %d (bytes) must be >= heads * 128, q 16-byte aligned", who, i, ldq[i]);
    IFX_REQUIRE(ldo[i] >= heads * 128 && ldo[i] % 8 == 0 && ((uintptr_t)it.out & 7) == 0, "%s: item %d: out row stride %d must be >= heads * 128 and %% 8",
                who, i, ldo[i]);
    big = big || (long long)it.num_slots * pitch >= (1ll << 31);
    q_rows[i] = it.q_rows, kv_len[i] = it.kv_len;
  }
  if (big) {
    set_error("%s: a cache of 2 GiB or more (byte offsets are 32-bit)", who);
    return IFX_EUNSUP;
  }
  kv8::MultiPlan p;
  if (kv8::plan_grouped_multi(q_rows, kv_len, n_items, heads, group_tokens, p) != IFX_OK) {      // (what is IFX_EINVAL there was refused above)
    set_error("%s: %d items x %d heads do not fit the raster table (%d streams, %d row tiles per XCD): launch them one by one", who, n_items,
              heads, kMultiStreams, kMaxTile0);
    return IFX_EUNSUP;
  }
  if (p.n_streams == 0) return IFX_OK;
  AttnKv8GroupedMultiArgs a{};
  for (int i = 0; i < n_items; ++i) {
    const int c = p.order[i];
    a.item[i] = AttnKv8GroupedItem{items[c].q8, (unsigned short*)items[c].out, items[c].k, items[c].v, items[c].v_scale, ldq[c], ldo[c], q_rows[c],
                                   kv_len[c], (q_rows[c] + kRows - 1) / kRows, kv8::grouped_key_tiles(group_tokens, kv_len[c])};
  }
  for (int i = n_items; i < kMultiItems; ++i) a.item[i] = a.item[0];      // never resolved: no raster word names them
  for (int s = 0; s < p.n_streams; ++s) a.stream[s] = (unsigned)p.tile0[s] << kTile0Shift | (unsigned)p.head[s] << kItemBits | (unsigned)p.item[s];
  for (int x = 0; x < kXcds; ++x) a.xcd_first[x] = p.xcd_first[x], a.xcd_tiles[x] = p.xcd_tiles[x];
  a.xcd_first[kXcds] = p.xcd_first[kXcds];
  a.group = heads / kv_heads, a.pitch = (int)pitch;
  a.tokens = group_tokens, a.tpg = (group_tokens + kKeys - 1) / kKeys, a.kv_heads = kv_heads;
  if (const int rc = launch_lds<attn_fwd_kv8_grouped_multi_kernel>(dim3(p.grid), dim3(512), kLds, (hipStream_t)stream, who, a)) return rc;
  return check_launch(who);
}

extern "C" int ifx_rmsnorm_rope_kv8_append_ring_multi(const ifx_kv8_ring_append_item* items, int32_t n_items, const ifx_bf16* wq, const ifx_bf16* wk,
                                                      int32_t kv_heads, int32_t head_dim, int32_t group_tokens, int32_t dim, float eps,
                                                      void* stream) {
  const char* who = "ifx_rmsnorm_rope_kv8_append_ring_multi";
  IFX_REQUIRE(items && n_items >= 1 && n_items <= kMultiItems, "%s: 1..%d items per launch (got %d)", who, kMultiItems, n_items);
  IFX_REQUIRE(wq && wk && dim > 0 && dim % 8 == 0, "%s: bad arguments", who);
  IFX_REQUIRE(kv_heads > 0 && (long long)kv_heads * head_dim == dim, "%s: kv_heads %d x head_dim %d does not match dim %d", who, kv_heads, head_dim, dim);
  IFX_REQUIRE(group_tokens > 0, "%s: groups of %d tokens", who, group_tokens);
  const int G = group_tokens;
  for (int i = 0; i < n_items; ++i) {
    const ifx_kv8_ring_append_item& it = items[i];
    IFX_REQUIRE(it.qkv && it.q8_out && it.rope && it.k && it.v && it.v_scale && it.rows >= 0 && it.qkv_row_stride % 8 == 0, "%s: item %d: bad arguments", who, i);
    IFX_REQUIRE(it.num_slots > 0 && it.num_slots % G == 0, "%s: item %d: %d slots are no whole number of groups of %d", who, i, it.num_slots, G);
    IFX_REQUIRE(it.ring_base >= 0 && it.ring_len > 0 && (long long)it.ring_base + it.ring_len <= it.num_slots,
                "%s: item %d: ring [%d, %d + %d) outside the cache's %d slots", who, i, it.ring_base, it.ring_base, it.ring_len, it.num_slots);
    IFX_REQUIRE(it.start >= 0 && it.rows <= it.ring_len, "%s: item %d: %d rows from position %d into a ring of %d slots", who, i, it.rows, it.start, it.ring_len);
    IFX_REQUIRE(it.start % G == 0 && it.ring_base % G == 0 && it.ring_len % G == 0 && it.rows % G == 0,
                "%s: item %d: start %d, ring_base %d, ring_len %d and rows %d must be whole frames of %d tokens (a frame is one scale group)", who, i,
                it.start, it.ring_base, it.ring_len, it.rows, G);
    IFX_REQUIRE(it.qkv_row_stride >= 3 * dim, "%s: item %d: qkv_row_stride (ld %d) must cover the 3 x dim (%d) columns read", who, i, it.qkv_row_stride, dim);
    IFX_REQUIRE(it.rope->flags == 0, "%s: item %d: rope flags %d (the V rows are always taken from qkv)", who, i, it.rope->flags);
    IFX_REQUIRE(it.rope->q_scale >= 0.f && it.rope->q_scale == it.rope->q_scale, "%s: item %d: q_scale must be >= 0 (0 = 1)", who, i);
  }
  if (head_dim != 128) {
    set_error("%s: head_dim %d (built for 128)", who, head_dim);
    return IFX_EUNSUP;
  }
  Kv8RingAppendMultiArgs a{};
  for (int i = 0; i < n_items; ++i) {
    const ifx_kv8_ring_append_item& it = items[i];
    Kv8RingAppendItem& d = a.item[i];
    if (const int rc = resolve_rope(who, it.rope, head_dim, dim, it.rows, &d.ra)) return rc;
    d.ra.q_scale = it.rope->q_scale > 0.f ? it.rope->q_scale : 1.0f;
    d.qkv = it.qkv, d.q8 = it.q8_out, d.k = it.k, d.v = it.v, d.v_scale = it.v_scale, d.ld = it.qkv_row_stride;
    d.ring_base = it.ring_base, d.ring_len = it.ring_len;
    d.start = it.start < it.ring_base ? it.start : it.ring_base + (it.start - it.ring_base) % it.ring_len;
    a.row0[i + 1] = a.row0[i] + it.rows;
    a.slab0[i + 1] = a.slab0[i] + it.rows / G * kv_heads;
  }
  for (int i = n_items; i < kMultiItems; ++i) a.item[i] = a.item[0], a.row0[i + 1] = a.row0[n_items], a.slab0[i + 1] = a.slab0[n_items];
  a.wq = wq, a.wk = wk, a.dim = dim, a.head_dim = head_dim, a.kv_heads = kv_heads, a.group_tokens = G, a.eps = eps;
  const int rows = a.row0[kMultiItems];
  if (rows == 0) return IFX_OK;
  return dispatch_nch<3, 4, 6>(dim, "ifx_rmsnorm_rope_kv8_append_ring_multi: dim %d is wider than the 3072 channels built", [&](auto nch) {
    hipLaunchKernelGGL(rmsnorm_rope_kv8_append_ring_multi_kernel<decltype(nch)::value>, dim3(a.slab0[kMultiItems] + (rows + 3) / 4), dim3(256), 0,
                       (hipStream_t)stream, a);
    return check_launch(who);
  });
}

// ---------------------------------------------------------------------------
// include/inferix_hip_kv8_magi.h
static const char* kRangesUnsup = "%s: %d ranges x %d kv heads do not fit the launch (%d ranges, %d streams, %d row tiles per XCD): launch them range by range";

extern "C" int ifx_attn_kv8_ranges_plan(const int32_t* q_ranges, const int32_t* k_ranges, int32_t n_ranges, int32_t heads, int32_t kv_heads,
                                        int32_t seg_split, ifx_kv8_ranges_plan* plan, int32_t* stream_range, int32_t* stream_kv_head,
                                        int32_t* stream_tile0, int32_t capacity) {
  const char* who = "ifx_attn_kv8_ranges_plan";
  IFX_REQUIRE(plan && stream_range && stream_kv_head && stream_tile0, "%s: bad arguments", who);
  kv8::RangesPlan p;
  const int rc = kv8::plan_ranges(q_ranges, k_ranges, n_ranges, heads, kv_heads, seg_split, p);
  if (rc == IFX_EUNSUP) set_error(kRangesUnsup, who, n_ranges, kv_heads, kRanges, kRangeStreams, kMaxTile0);
  IFX_REQUIRE(rc != IFX_EINVAL, "%s: bad arguments (n_ranges >= 1, heads a multiple of kv_heads, query ranges ordered, key ranges not empty, seg_split >= 0)", who);
  if (rc) return rc;
  IFX_REQUIRE(capacity >= p.n_streams, "%s: %d streams, room for %d", who, p.n_streams, capacity);
  *plan = ifx_kv8_ranges_plan{};
  plan->n_streams = p.n_streams, plan->grid = p.grid, plan->lds_bytes = kLds, plan->arg_bytes = (int)sizeof(AttnKv8RangesArgs);
  for (int i = 0; i < n_ranges; ++i) plan->order[i] = p.order[i], plan->key_tiles[i] = p.key_tiles[i];
  for (int x = 0; x < kXcds; ++x) plan->xcd_first[x] = p.xcd_first[x], plan->xcd_tiles[x] = p.xcd_tiles[x], plan->xcd_cost[x] = p.xcd_cost[x];
  plan->xcd_first[kXcds] = p.xcd_first[kXcds];
  for (int s = 0; s < p.n_streams; ++s) stream_range[s] = p.order[p.range[s]], stream_kv_head[s] = p.kv_head[s], stream_tile0[s] = p.tile0[s];
  return IFX_OK;
}

extern "C" int ifx_attn_fwd_kv8_ranges(const uint8_t* q8, int32_t ldq, ifx_bf16* out, int32_t ldo, const uint8_t* k, const uint8_t* v,
                                       const float* v_scale, int32_t num_slots, int32_t kv_heads, int32_t seg_split, int32_t seg_base,
                                       int32_t q_rows, int32_t heads, int32_t n_ranges, const int32_t* q_ranges, const int32_t* k_ranges,
                                       void* stream) {
  const char* who = "ifx_attn_fwd_kv8_ranges";
  IFX_REQUIRE(q8 && out && k && v && v_scale && q_ranges && k_ranges && q_rows >= 0 && heads > 0 && n_ranges >= 1 && num_slots > 0, "%s: bad arguments", who);
  IFX_REQUIRE(kv_heads > 0 && heads % kv_heads == 0, "%s: heads %d is no multiple of kv_heads %d", who, heads, kv_heads);
  IFX_REQUIRE(seg_split >= 0 && (seg_split == 0 || (seg_base >= seg_split && seg_base <= num_slots)),
              "%s: seg_split %d / seg_base %d (0 <= seg_split <= seg_base <= %d slots)", who, seg_split, seg_base, num_slots);
  if (ldq == 0) ldq = heads * 128;
  if (ldo == 0) ldo = heads * 128;
  IFX_REQUIRE(ldq >= heads * 128 && ldq % 16 == 0 && ((uintptr_t)q8 & 15) == 0, "%s: q row stride %d (bytes) must be >= heads * 128, q 16-byte aligned", who, ldq);
  IFX_REQUIRE(ldo >= heads * 128 && ldo % 8 == 0 && ((uintptr_t)out & 7) == 0, "%s: out row stride %d must be >= heads * 128 and %% 8", who, ldo);
  if (n_ranges > kRanges) {
    set_error(kRangesUnsup, who, n_ranges, kv_heads, kRanges, kRangeStreams, kMaxTile0);
    return IFX_EUNSUP;
  }
  AttnKv8RangesArgs a{};
  AttnKv8Range rg[kRanges];
  for (int i = 0; i < n_ranges; ++i) {
    const int qs = q_ranges[2 * i], qe = q_ranges[2 * i + 1], ks = k_ranges[2 * i], ke = k_ranges[2 * i + 1];
    IFX_REQUIRE(qs >= 0 && qe >= qs && qe <= q_rows, "%s: query range %d = [%d, %d) outside the %d rows", who, i, qs, qe, q_rows);
    IFX_REQUIRE(ks >= 0 && ke > ks, "%s: key range %d = [%d, %d) is empty or negative", who, i, ks, ke);
    AttnKv8Range& r = rg[i];
    r.q0 = qs, r.q_rows = qe - qs, r.row_tiles = (qe - qs + kRows - 1) / kRows;
    kv8::seg_runs(ks, ke, seg_split, seg_base, r);
    // (the first run ends at seg_split <= seg_base <= num_slots when there is a map)
    IFX_REQUIRE(r.a1 <= num_slots && r.b1 <= num_slots, "%s: key range %d = [%d, %d) maps outside the cache's %d slots (seg_split %d, seg_base %d)", who, i,
                ks, ke, num_slots, seg_split, seg_base);
  }
  const long long pitch = (long long)kv_heads * 128;
  if ((long long)num_slots * pitch >= (1ll << 31)) {
    set_error("%s: a cache of %lld bytes (byte offsets are 32-bit: caches below 2 GiB)", who, num_slots * pitch);
    return IFX_EUNSUP;
  }
  kv8::RangesPlan p;
  if (kv8::plan_ranges(q_ranges, k_ranges, n_ranges, heads, kv_heads, seg_split, p) != IFX_OK) {      // (what is IFX_EINVAL there was refused above)
    set_error(kRangesUnsup, who, n_ranges, kv_heads, kRanges, kRangeStreams, kMaxTile0);
    return IFX_EUNSUP;
  }
  if (p.n_streams == 0) return IFX_OK;
  a.q = q8, a.out = (unsigned short*)out, a.k = k, a.v = v, a.v_scale = v_scale;
  a.ldq = ldq, a.ldo = ldo, a.group = heads / kv_heads, a.pitch = (int)pitch;
  for (int i = 0; i < n_ranges; ++i) a.range[i] = rg[p.order[i]];
  for (int i = n_ranges; i < kRanges; ++i) a.range[i] = a.range[0];      // never resolved: no raster word names them
  for (int s = 0; s < p.n_streams; ++s) a.stream[s] = (unsigned)p.tile0[s] << kTile0Shift | (unsigned)p.kv_head[s] << kItemBits | (unsigned)p.range[s];
  for (int x = 0; x < kXcds; ++x) a.xcd_first[x] = p.xcd_first[x], a.xcd_tiles[x] = p.xcd_tiles[x];
  a.xcd_first[kXcds] = p.xcd_first[kXcds];
  if (const int rc = launch_lds<attn_fwd_kv8_ranges_kernel>(dim3(p.grid), dim3(512), kLds, (hipStream_t)stream, who, a)) return rc;
  return check_launch(who);
}

// Host-side launch plan of the 8-bit self-attention kernel (ifx_attn_kv8.hip): tile sizes, the ring, the LDS layout of a slot and the
// per-XCD raster, shared by the launcher, the kernel (the constants) and ifx_attn_kv8_plan.  No GPU call.
#pragma once
#include "../../include/inferix_hip_kv8.h"

namespace ifx {
namespace kv8 {

constexpr int kRows = 256;                 // query rows per workgroup: 8 waves x one 32-row MFMA block
constexpr int kKeys = 64;                  // keys per tile: two 32-key score blocks = ONE K = 64 step of the PV product
constexpr int kRing = 3;                   // slots: tile t is computed while t + 1 is being transposed and t + 2 is in flight
constexpr int kKTile = kKeys * 128;        // K tile as it lies in the cache: 64 rows x 128 B, 16-byte chunks XOR-swizzled by (row >> 1) & 7
// V tile TRANSPOSED: 128 channel rows x 64 key bytes, 16 B of padding after every 4 rows (the transposing stores of one wave go to
// rows 4 c + e, c = 0 .. 31: without the padding all of them would fall into one bank)
constexpr int kVtTile = 128 * kKeys + 32 * 16;
constexpr int kSlot = kKTile + kVtTile;
constexpr int kLds = kRing * kSlot;

inline bool plan(int q_rows, int heads, int kv_start, int kv_len, ifx_kv8_plan* p) {
  if (!p || q_rows <= 0 || heads <= 0 || kv_start < 0 || kv_len <= kv_start) return false;
  p->row_tiles = (q_rows + kRows - 1) / kRows;
  p->key_tiles = (kv_len - kv_start + kKeys - 1) / kKeys;
  p->per_xcd = (p->row_tiles * heads + 7) / 8;
  p->grid = 8 * p->per_xcd;
  p->ring = kRing;
  p->lds_bytes = kLds;
  return true;
}

}  // namespace kv8
}  // namespace ifx

// ifx_attn_fwd_multi: the kernels' argument struct and the launch plan (host arithmetic, no GPU call) — the multi-range launch of
// ifx_attn.h generalised from "ranges of one cache" to "one cache per range".  A struct of its own: AttnArgsPP is a by-value kernel
// argument of every attn_fwd_pp_kernel, so growing it would change all their descriptors.
#pragma once
#include "../../include/inferix_hip_sessions.h"
#include "ifx_attn.h"

namespace ifx {

constexpr int kAttnMultiItems = IFX_ATTN_MULTI_MAX_ITEMS;

// One item as the kernel reads it: the arguments of that item's own unsplit launch that differ between items.
struct AttnItemArgs {
  const unsigned short* q;
  unsigned short* out;
  const unsigned short* k;
  const unsigned short* v;
  const int32_t* pt;        // page table (PAGED = 1 instantiations), else nullptr
  int ps;                   // page size
  unsigned ps_magic;        // floor(2^32 / page_size) + 1 (AttnArgsPP::ps_magic)
  int q_rows, kv_start, kv_len, num_slots;
  int ldq, ldo;
};
struct AttnMultiArgs {
  AttnItemArgs item[kAttnMultiItems];   // in launch order: longest key range first
  int rt0[kAttnMultiItems + 1];         // q tile ids [rt0[i], rt0[i + 1]) of a head belong to item[i]
  int n_items, heads, kv_heads, q_per_kv;
  int total;                            // workgroups: rt0[n_items] * heads, tile-major
  float scale, scale_log2;
  unsigned* dbg_rescales;               // AttnArgsPP::dbg_rescales
};

// What a checked request comes to under option values `variant` and `mfma`: the kernel arguments, order[i] = the caller's index of
// item[i], the schedule (6 or 7), the page kind (0 contiguous, 1 wave-uniform translation) and the loop form.
//   schedule: 6 / 7 as named; auto picks between them by the items' mean row count over heads * n_items K/V streams (the rule of
//             the range launch); 1 .. 5 are not built for this launch.
//   form:     pre as a single launch decides it; mfma16 from the LONGEST item's key count (one launch, one form).
inline int attn_plan_multi(const ifx_attn_item* items, int n, int heads, float scale, int variant, int mfma, unsigned* dbg,
                           AttnMultiArgs& a, int* order, int& schedule, int& paged, AttnForm& form) {
  if (n < 1 || n > kAttnMultiItems) {
    set_error("ifx_attn_fwd_multi: 1..%d items per launch (got %d)", kAttnMultiItems, n);
    return IFX_EINVAL;
  }
  if (variant != 0 && variant != 6 && variant != 7) {
    set_error("ifx_attn_fwd_multi: built for attn_variant 6 and 7 (and 0, which picks between them), not %d", variant);
    return IFX_EUNSUP;
  }
  long long rows = 0;
  int longest = 0;
  paged = -1;
  for (int i = 0; i < n; ++i) {
    const ifx_kv_view* kv = items[i].kv;
    if (kv->kv_heads != items[0].kv->kv_heads) {
      set_error("ifx_attn_fwd_multi: item %d has kv_heads %d, item 0 has %d", i, kv->kv_heads, items[0].kv->kv_heads);
      return IFX_EINVAL;
    }
    int kind = 0;
    unsigned magic = 0;
    if (kv->page_table != nullptr) {
      magic = (kv->page_size >= 2 && (long long)kv->num_slots * kv->page_size < (1ll << 32)) ? (unsigned)((1ull << 32) / (unsigned)kv->page_size) + 1u : 0u;
      if (kv->page_size < 3 || magic == 0) {
        set_error("ifx_attn_fwd_multi: item %d needs per-lane page translation (page_size %d), which is not built for this launch", i, kv->page_size);
        return IFX_EUNSUP;
      }
      kind = 1;
    } else if (kv->seg_split > 0) {
      set_error("ifx_attn_fwd_multi: item %d is a two-segment view (seg_split %d), which is not built for this launch", i, kv->seg_split);
      return IFX_EUNSUP;
    }
    if (paged >= 0 && kind != paged) {
      set_error("ifx_attn_fwd_multi: item %d is %s and item 0 is not: one launch takes views of one kind", i, kind ? "paged" : "contiguous");
      return IFX_EUNSUP;
    }
    paged = kind;
    rows += items[i].q_rows;
    longest = max(longest, items[i].kv_len - items[i].kv_start);
    order[i] = i;
  }
  schedule = attn_pick_variant(variant, (int)(rows / n), heads * n);
  const int QT = attn_schedule(schedule).qt;
  // longest key ranges first (stable): tile ids are handed out in order, so the expensive tiles must not be the tail of the launch
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && items[order[j]].kv_len - items[order[j]].kv_start > items[order[j - 1]].kv_len - items[order[j - 1]].kv_start; --j) {
      const int t = order[j];
      order[j] = order[j - 1];
      order[j - 1] = t;
    }
  a = AttnMultiArgs{};
  for (int i = 0; i < n; ++i) {
    const ifx_attn_item& it = items[order[i]];
    const ifx_kv_view* kv = it.kv;
    AttnItemArgs& d = a.item[i];
    d.q = it.q, d.out = it.out, d.k = kv->k, d.v = kv->v;
    d.pt = kv->page_table;
    d.ps = kv->page_size;
    d.ps_magic = kv->page_table ? (unsigned)((1ull << 32) / (unsigned)kv->page_size) + 1u : 0u;
    d.q_rows = it.q_rows, d.kv_start = it.kv_start, d.kv_len = it.kv_len, d.num_slots = kv->num_slots;
    d.ldq = it.ldq > 0 ? it.ldq : heads * 128;
    d.ldo = it.ldo > 0 ? it.ldo : heads * 128;
    a.rt0[i + 1] = a.rt0[i] + (it.q_rows + QT - 1) / QT;
  }
  for (int i = n; i < kAttnMultiItems; ++i) a.rt0[i + 1] = a.rt0[n];
  a.n_items = n;
  a.heads = heads;
  a.kv_heads = items[0].kv->kv_heads;
  a.q_per_kv = heads / a.kv_heads;
  a.total = a.rt0[n] * heads;
  a.scale = scale > 0.f ? scale : 0.08838834764831845f;   // 1/sqrt(128)
  a.scale_log2 = a.scale * 1.4426950408889634f;
  a.dbg_rescales = dbg;
  form.pre = fabsf(a.scale_log2 - 1.0f) <= 2.5e-7f;
  form.mfma16 = attn_pick_mfma16(mfma, schedule, form.pre, false, longest);
  return IFX_OK;
}

int launch_attn_multi(const AttnMultiArgs& a, const AttnSchedule& s, int paged, AttnForm form, hipStream_t stream);   // ifx_attn_pp.hip

}  // namespace ifx

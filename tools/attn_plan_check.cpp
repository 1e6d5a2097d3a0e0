// The attention launch plan (ifx::attn_plan and the split heuristic of inferix_amd/csrc/ifx_attn.hip) as a stand-alone host program, so
// that its arithmetic can run under the host sanitizers without a GPU and without loading the library into another process:
//   make -C inferix_amd/csrc plan_check        (hipcc ... -Xarch_host -fsanitize=address,undefined; builds and runs it)
// Plans every attn_variant at the shapes of tests/test_cabi_and_host.py (ATTN_PLAN_SHAPES), as self-contained, split and partial
// launches over contiguous, paged (page sizes 64, 7, 2) and two-segment views, plus an 8-range launch; prints one line per variant
// (a checksum of the plans: equal between two builds that plan alike) and exits 0.  Launches nothing.
#include "../inferix_amd/csrc/ifx_attn.hip"
#include "check_stubs.h"

static int g_variant = 0;
namespace ifx {   // what the library's other files provide
void set_error(const char*, ...) {}
int attn_variant() { return g_variant; }
int attn_mfma() { return 0; }
unsigned* attn_debug_counter() { return nullptr; }
int launch_attn_pp(const AttnArgsPP&, const AttnSchedule&, int, bool, AttnForm, dim3, hipStream_t) { return IFX_OK; }
int launch_attn_merge(const float*, int, int, unsigned short*, float*, int, int, hipStream_t, int) { return IFX_OK; }
int launch_attn_multi(const AttnMultiArgs&, const AttnSchedule&, int, AttnForm, hipStream_t) { return IFX_OK; }
}  // namespace ifx

int main() {
  static const int shapes[12][4] = {{4680, 12, 0, 32760}, {585, 12, 0, 32760}, {585, 12, 0, 4680},   {585, 12, 4680, 9360},
                                    {1170, 12, 0, 32760}, {10800, 12, 0, 75600}, {12150, 3, 0, 48600}, {600, 12, 0, 6277},
                                    {300, 12, 0, 2048},   {130, 12, 0, 1000},    {585, 12, 0, 512},    {0, 12, 0, 100}};
  static unsigned short mem[64];
  static int32_t table[4096];
  ifx_kv_view views[5] = {};
  const int page_sizes[5] = {0, 64, 7, 2, 0};
  for (int i = 0; i < 5; ++i) {
    views[i].k = views[i].v = mem;
    views[i].page_table = page_sizes[i] ? table : nullptr;
    views[i].page_size = page_sizes[i] ? page_sizes[i] : 1;
    views[i].num_slots = 80000;
    views[i].kv_heads = 3;
    views[i].head_dim = 128;
    views[i].seg_split = i == 4 ? 1000 : 0;
    views[i].seg_delta = i == 4 ? 64 : 0;
  }
  const int q_ranges[16] = {0, 1500, 1500, 3000, 3000, 4500, 4500, 6000, 6000, 7500, 7500, 9000, 9000, 10500, 10500, 12150};
  const int k_ranges[16] = {0, 9000, 0, 40000, 100, 20000, 7, 48600, 0, 64, 30000, 30001, 5, 4700, 0, 48600};
  for (g_variant = 0; g_variant <= 7; ++g_variant) {
    unsigned long long sum = 0;
    int plans = 0;
    auto plan = [&](const ifx::AttnLaunch& L) {
      ifx::AttnArgsPP a = {};
      int schedule = 0, paged = 0;
      ifx::AttnForm form, form2;
      if (ifx::attn_plan(L, g_variant, 0, a, schedule, paged, form) != IFX_OK) return;
      ifx::attn_plan(L, g_variant, 2, a, schedule, paged, form2);      // attn_mfma 2: the 16x16x32 form on schedule 7 and nowhere else
      if (form2.mfma16 != (schedule == 7) || form2.pre != form.pre || (form.mfma16 && !(schedule == 7 && form.pre && a.splits == 1 && L.slot_cap == 0))) { printf("attn_mfma 2: form of schedule %d\n", schedule); exit(1); }
      const long long v[] = {schedule, paged, a.per_xcd, a.q_tiles, a.total,
                             a.splits, a.chunk_tiles, a.kv_start, a.kv_len, a.n_ranges, a.ps_magic, a.part_lse - a.part_o,
                             a.n_ranges ? a.rt0[a.n_ranges] + a.rk1[0] + a.rq0[a.n_ranges - 1] : 0};
      for (long long x : v) sum = sum * 1000003ull + (unsigned long long)x;
      ++plans;
    };
    for (const auto& s : shapes)
      for (const ifx_kv_view& kv : views) {
        int64_t bytes = 0;
        const int splits = ifx_attn_split_plan(s[0], s[1], s[2], s[3], &bytes);
        sum = sum * 1000003ull + (unsigned long long)splits + (unsigned long long)bytes;
        if (s[0] == 0) continue;
        static float ws[4];
        ifx::AttnLaunch L;
        L.q = mem, L.out = mem, L.kv = &kv, L.q_rows = s[0], L.heads = s[1], L.kv_start = s[2], L.kv_len = s[3];
        plan(L);                                    // unsplit, default scale
        L.scale = 0.6931471805599453f;              // scale * log2(e) = 1: the exponent forms
        L.splits = splits, L.workspace = ws;
        plan(L);                                    // as planned
        L.splits = 64;
        plan(L);                                    // more chunks than tiles allow
        L.out = nullptr, L.splits = 3, L.slot_base = 2, L.slot_cap = 8;
        plan(L);                                    // partial
        L.slot_base = 7;
        plan(L);                                    // slots beyond the workspace's: refused
      }
    for (const ifx_kv_view& kv : views)
      for (int n = 1; n <= 8; ++n) {
        ifx::AttnLaunch L;
        L.q = mem, L.out = mem, L.kv = &kv, L.q_rows = 12150, L.heads = 3, L.ldq = L.ldo = 3 * 128 + 64;
        L.n_ranges = n, L.q_ranges = q_ranges, L.k_ranges = k_ranges;
        plan(L);
      }
    printf("attn_variant %d: %d plans, checksum %016llx\n", g_variant, plans, sum);
  }
  return 0;
}

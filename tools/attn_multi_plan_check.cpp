// The launch plan of ifx_attn_fwd_multi (ifx::attn_plan_multi, inferix_amd/csrc/ifx_attn_multi.h) as a stand-alone host program, in the
// style of attn_plan_check.cpp: it runs under the host sanitizers without a GPU (make -C inferix_amd/csrc plan_check) and launches nothing.
// Checks, and prints one line per scenario:
//   * every item's kernel arguments are those attn_plan gives that item's OWN single unsplit launch (pointers, strides, key range,
//     capacity, page magic, tile count, scale, page kind, schedule and exponent form under a forced attn_variant);
//   * tiles are handed out longest key range first, equal ranges in the caller's order, and the tile table is their prefix sum;
//   * one loop form per launch: the matrix instruction follows the LONGEST item under attn_mfma 0, the option under 1 / 2;
//   * what is not built is refused with its code.
// Exit 0 when everything holds; a failed check prints what differed and exits 1.
#include "../inferix_amd/csrc/ifx_attn.hip"
#include "check_stubs.h"

#include <stdarg.h>
#include <string.h>

static int g_variant = 0;
static char g_error[512];
namespace ifx {   // what the library's other files provide
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}
int attn_variant() { return g_variant; }
int attn_mfma() { return 0; }
unsigned* attn_debug_counter() { return nullptr; }
int launch_attn_pp(const AttnArgsPP&, const AttnSchedule&, int, bool, AttnForm, dim3, hipStream_t) { return IFX_OK; }
int launch_attn_merge(const float*, int, int, unsigned short*, float*, int, int, hipStream_t, int) { return IFX_OK; }
int launch_attn_multi(const AttnMultiArgs&, const AttnSchedule&, int, AttnForm, hipStream_t) { return IFX_OK; }
}  // namespace ifx

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      printf("FAILED %s: ", #cond);      \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
      exit(1);                           \
    }                                    \
  } while (0)

static unsigned short mem[8][64];
static int32_t table[4096];

static ifx_kv_view view(int kind, int slots, int kv_heads = 12) {   // kind 0 contiguous, > 0: page size, < 0: two segments
  ifx_kv_view v = {};
  v.k = mem[0], v.v = mem[1];
  v.page_table = kind > 0 ? table : nullptr;
  v.page_size = kind > 0 ? kind : 1;
  v.num_slots = slots, v.kv_heads = kv_heads, v.head_dim = 128;
  v.seg_split = kind < 0 ? 100 : 0, v.seg_delta = kind < 0 ? 8 : 0;
  return v;
}

// plans `n` items and checks each against its own single launch; returns the order as a string
static std::string plan(const char* what, const ifx_attn_item* items, int n, int heads, float scale, int variant, int mfma, int want_schedule,
                        bool want_m16) {
  ifx::AttnMultiArgs a;
  int order[8], schedule = 0, paged = 0;
  ifx::AttnForm form;
  const int rc = ifx::attn_plan_multi(items, n, heads, scale, variant, mfma, nullptr, a, order, schedule, paged, form);
  CHECK(rc == IFX_OK, "%s: rc %d %s", what, rc, g_error);
  CHECK(schedule == want_schedule && form.mfma16 == want_m16, "%s: schedule %d (want %d), mfma16 %d (want %d)", what, schedule, want_schedule,
        form.mfma16, want_m16);
  const int QT = ifx::attn_schedule(schedule).qt;
  std::string ord;
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    const ifx_attn_item& it = items[order[i]];
    const ifx::AttnItemArgs& d = a.item[i];
    ord += (char)('0' + order[i]);
    if (i > 0) {
      const ifx_attn_item& prev = items[order[i - 1]];
      const int kp = prev.kv_len - prev.kv_start, kc = it.kv_len - it.kv_start;
      CHECK(kp > kc || (kp == kc && order[i - 1] < order[i]), "%s: item %d (%d keys) behind item %d (%d keys)", what, order[i], kc, order[i - 1], kp);
    }
    CHECK(a.rt0[i] == tiles, "%s: rt0[%d] = %d, want %d", what, i, a.rt0[i], tiles);
    tiles += (it.q_rows + QT - 1) / QT;
    // the item alone, under the schedule of the launch
    ifx::AttnLaunch L;
    L.q = (const unsigned short*)it.q, L.out = (unsigned short*)it.out, L.kv = it.kv, L.q_rows = it.q_rows, L.heads = heads;
    L.ldq = it.ldq, L.ldo = it.ldo, L.kv_start = it.kv_start, L.kv_len = it.kv_len, L.scale = scale;
    ifx::AttnArgsPP s = {};
    int s_schedule = 0, s_paged = 0;
    ifx::AttnForm s_form;
    CHECK(ifx::attn_plan(L, schedule, mfma, s, s_schedule, s_paged, s_form) == IFX_OK, "%s: single plan of item %d", what, order[i]);
    CHECK(s_schedule == schedule && s_paged == paged && s_form.pre == form.pre, "%s: item %d alone: schedule %d paged %d pre %d", what, order[i],
          s_schedule, s_paged, s_form.pre);
    CHECK(d.q == s.q && d.out == s.out && d.k == s.k && d.v == s.v && d.pt == s.ka.pt && d.ps == s.ka.ps && d.ps_magic == s.ps_magic &&
              d.q_rows == s.q_rows && d.kv_start == s.kv_start && d.kv_len == s.kv_len && d.num_slots == s.num_slots && d.ldq == s.ldq &&
              d.ldo == s.ldo && a.rt0[i + 1] - a.rt0[i] == s.q_tiles && a.scale == s.scale && a.scale_log2 == s.scale_log2 &&
              a.kv_heads == s.kv_heads && a.q_per_kv == s.q_per_kv && s.splits == 1 && s.n_ranges == 0,
          "%s: the arguments of item %d differ from its single launch's", what, order[i]);
  }
  CHECK(a.rt0[n] == tiles && a.total == tiles * heads && a.n_items == n && a.heads == heads, "%s: %d tiles x %d heads, total %d", what, tiles, heads, a.total);
  printf("%-34s variant %d mfma %d: schedule %d %s%s page kind %d, order %s, %d tiles x %d heads\n", what, variant, mfma, schedule,
         form.pre ? "pre " : "", form.mfma16 ? "16x16x32" : "32x32x16", paged, ord.c_str(), tiles, heads);
  return ord;
}

static void refused(const char* what, const ifx_attn_item* items, int n, int heads, int variant, int want_rc, const char* text) {
  ifx::AttnMultiArgs a;
  int order[8], schedule = 0, paged = 0;
  ifx::AttnForm form;
  g_error[0] = 0;
  const int rc = ifx::attn_plan_multi(items, n, heads, 0.f, variant, 0, nullptr, a, order, schedule, paged, form);
  CHECK(rc == want_rc && strstr(g_error, text), "%s: rc %d (want %d), message '%s' (want '%s')", what, rc, want_rc, g_error, text);
  printf("%-34s refused (%d): %s\n", what, rc, g_error);
}

int main() {
  const float LN2 = 0.6931471805599453f;      // scale * log2(e) = 1: the exponent forms
  ifx_kv_view cont[8], paged64[8];
  const int keys[8] = {4680, 14040, 32760, 23400, 9360, 32760, 18720, 28080};
  ifx_attn_item it[9] = {}, pg[8] = {};
  for (int i = 0; i < 8; ++i) {
    cont[i] = view(0, 32760);
    cont[i].k = mem[i], cont[i].v = mem[(i + 1) % 8];
    paged64[i] = view(64, 32768);
    it[i] = ifx_attn_item{mem[i], 0, mem[7 - i], 0, &cont[i], 4680, 0, keys[i]};
    pg[i] = ifx_attn_item{mem[i], 1536 + 64, mem[7 - i], 3 * 1536, &paged64[i], 4680 - 7 * i, i == 3 ? 1560 : 0, keys[i]};
  }
  it[8] = it[0];
  // the shape of tools/bench_sessions.py: four sessions of 4680 rows at different positions of their videos
  CHECK(plan("4 sessions, 480p", it, 4, 12, LN2, 0, 0, 7, true) == "2310", "order");
  CHECK(plan("4 sessions, 480p", it, 4, 12, LN2, 7, 1, 7, false) == "2310", "order");
  CHECK(plan("4 sessions, 480p", it, 4, 12, LN2, 6, 2, 6, false) == "2310", "order");
  CHECK(plan("4 sessions, unscaled q", it, 4, 12, 0.f, 0, 0, 7, false) == "2310", "order");
  CHECK(plan("8 sessions, equal key counts", it, 8, 12, LN2, 0, 0, 6, false) == "25736140", "order");   // 3552 128-row tiles: 7 rounds of 512 against 8 of 256
  CHECK(plan("8 sessions, equal key counts", it, 8, 12, LN2, 7, 0, 7, true) == "25736140", "order");
  CHECK(plan("1 session", it + 1, 1, 12, LN2, 7, 2, 7, true) == "0", "order");
  CHECK(plan("2 short sessions", it, 2, 12, LN2, 7, 0, 7, true) == "10", "order");      // longest 14040 keys: 16x16x32 for both items
  CHECK(plan("paged, strided, ragged rows", pg, 8, 12, LN2, 0, 0, 6, false) == "25736140", "order");
  CHECK(plan("paged, strided, ragged rows", pg, 5, 12, LN2, 6, 0, 6, false) == "23140", "order");
  {                                            // one sequence-parallel-sized row count: the automatic choice takes the 128-row tiles
    ifx_attn_item sp[4];
    for (int i = 0; i < 4; ++i) sp[i] = it[i], sp[i].q_rows = 585;
    plan("4 x 585 rows", sp, 4, 12, LN2, 0, 0, 6, false);
  }
  // refusals
  refused("no items", it, 0, 12, 7, IFX_EINVAL, "1..8 items per launch (got 0)");
  refused("nine items", it, 9, 12, 7, IFX_EINVAL, "1..8 items per launch (got 9)");
  for (int v = 1; v <= 5; ++v) refused("a schedule that is not built", it, 2, 12, v, IFX_EUNSUP, "built for attn_variant 6 and 7");
  ifx_kv_view seg = view(-1, 32760), ps2 = view(2, 32760), ps1 = view(1, 32760), h6 = view(0, 32760, 6);
  ifx_attn_item bad[2] = {it[0], it[1]};
  bad[1].kv = &seg;
  refused("two-segment view", bad, 2, 12, 7, IFX_EUNSUP, "item 1 is a two-segment view");
  bad[1].kv = &ps2;
  refused("two-row pages", bad, 2, 12, 7, IFX_EUNSUP, "item 1 needs per-lane page translation (page_size 2)");
  bad[1].kv = &ps1;
  refused("one-row pages", bad, 2, 12, 7, IFX_EUNSUP, "item 1 needs per-lane page translation (page_size 1)");
  bad[1].kv = &paged64[1];
  refused("mixed view kinds", bad, 2, 12, 7, IFX_EUNSUP, "item 1 is paged and item 0 is not");
  bad[0].kv = &paged64[0], bad[1].kv = &cont[1];
  refused("mixed view kinds", bad, 2, 12, 7, IFX_EUNSUP, "item 1 is contiguous and item 0 is not");
  bad[0].kv = &cont[0], bad[1].kv = &h6;
  refused("differing kv_heads", bad, 2, 12, 7, IFX_EINVAL, "item 1 has kv_heads 6, item 0 has 12");
  printf("attn_multi_plan_check: ok\n");
  return 0;
}

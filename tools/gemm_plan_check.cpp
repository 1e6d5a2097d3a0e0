// The GEMM dispatch (ifx::gemm_plan / gemm_q8_plan of inferix_amd/csrc/ifx_gemm_plan.h behind the entry points of ifx_gemm.hip and
// ifx_quant.hip) as a stand-alone host program, so that the whole decision can run without a GPU, under the host sanitizers, and
// without loading the library into another process:
//   make -C inferix_amd/csrc plan_check        (hipcc ... -Xarch_host -fsanitize=address,undefined; builds and runs it)
// It calls the real entry points with every gemm_variant 0 - 29 x gemm_small_split 0 / 1 over a grid of shapes, epilogues, operand
// alignments and workspace offers; what the other files of the library provide is stubbed, and every launch is recorded instead of
// made, as one canonical line:
//   a cross-file launcher  : `path tile tj ks workspace-used y2`    (path = dma | w4 | pp | pp-f8 | pp-i8; - = does not apply)
//   a kernel of the entry point's own file (register-staged, the 8-bit LDS-DMA tiles): `local <kernel instantiation> grid block lds`
//   a refusal              : `rc <code> <format string of the error>`
// "workspace-used" is 1 only when the kernel reads or writes the workspace (ks != 1), whatever pointer the launcher was handed.
// Prints one checksum line per (small_split, variant, entry point) — the two workspace queries are folded in — and, in full, the lines
// of the project's named shapes under the automatic choice; tests/test_cabi_and_host.py compares the output with the recorded one.
#include <string>

#include "../inferix_amd/csrc/ifx_gemm.hip"
#include "../inferix_amd/csrc/ifx_quant.hip"
#include "check_stubs.h"

static int g_variant = 0, g_small_split = 0;
static std::string g_launch, g_error;

static void record(const char* path, int tile, int tj, int ks, bool y2) {
  char b[96], t[3][16];
  const int v[3] = {tile, tj, ks};
  for (int i = 0; i < 3; ++i) v[i] < 0 ? (void)snprintf(t[i], 16, "-") : (void)snprintf(t[i], 16, "%d", v[i]);
  snprintf(b, sizeof b, "%s %s %s %s %d %d", path, t[0], t[1], t[2], ks >= 0 && ks != 1, (int)y2);
  g_launch += g_launch.empty() ? "" : " + ";
  g_launch += b;
}

// the runtime calls a launch of the entry point's own file makes (kernel<<<...>>> = push the configuration, pop it in the kernel's host
// stub, launch): the launch is named and measured, not made
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  const std::string name = kernel_name(f);
  char b[64];
  snprintf(b, sizeof b, " %u %u %zu", grid.x, block.x, lds);
  g_launch += (g_launch.empty() ? "local " : " + local ") + name + b;
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetDeviceCount(int* n) { return *n = 1, hipSuccess; }      // the opt-in is per device (ifx_launch.h): one, never asked for

namespace ifx {   // what the library's other files provide
void set_error(const char* fmt, ...) { g_error = fmt; }
int gemm_variant() { return g_variant; }
int gemm_small_split() { return g_small_split; }
int launch_gemm_lds_dma(int tile, const unsigned short*, int, const unsigned short*, unsigned short*, int, int, int, int, int,
                        const EpiArgs&, hipStream_t) {
  record("dma", tile, -1, -1, false);
  return IFX_OK;
}
int launch_gemm_w4(const unsigned short*, int, const unsigned short*, unsigned short*, int, int, int, int, int, const EpiArgs&,
                   hipStream_t, int splits, void* workspace) {
  record((splits > 1) == (workspace != nullptr) ? "w4" : "w4-WORKSPACE-MISMATCH", -1, -1, splits, false);
  return IFX_OK;
}
// the plan's ks decides; a workspace pointer goes with a split and with nothing else
int launch_gemm_pp(const unsigned short*, int, const unsigned short*, unsigned short*, int, int, int, int, int, const EpiArgsP& ea,
                   hipStream_t, int tj, int ks, void* workspace, int q8_int8) {
  const char* path = ea.sa == nullptr ? "pp" : q8_int8 ? "pp-i8" : "pp-f8";
  record((ks != 1) == (workspace != nullptr) ? path : "pp-WORKSPACE-MISMATCH", -1, tj, ks, ea.y2 != nullptr);
  return IFX_OK;
}
}  // namespace ifx

// ------------------------------------------------------------------------------------------------------------------------------------
alignas(64) static unsigned char g_mem[4096];   // operand addresses only: no launch is made, nothing is read or written
static unsigned short* at(int off) { return (unsigned short*)(g_mem + off); }
static unsigned long long g_sum;
static int g_calls;
static std::string g_last;

static void fold(const std::string& s) {
  for (unsigned char c : s) g_sum = (g_sum ^ c) * 1099511628211ull;
  g_sum = (g_sum ^ 10) * 1099511628211ull;
}
static void begin() { g_launch.clear(), g_error.clear(); }
static void end(int rc) {
  g_last = rc != IFX_OK ? "rc " + std::to_string(rc) + " " + g_error : g_launch.empty() ? "no launch" : g_launch;
  fold(g_last);
  ++g_calls;
}

enum Epi { BIAS, GELU, RESIDUAL, GATE1560, GATE40, GATE100, N_EPI };
enum Operands { IDEAL, LDY4, RES8, BIAS4, N_OPERANDS };
static const char* const kEpiName[N_EPI] = {"bias", "gelu", "residual", "gate/1560", "gate/40", "gate/100"};

static ifx_epilogue epilogue(int e, int op, int N) {
  ifx_epilogue epi = {};
  epi.epilogue = e == BIAS ? IFX_EPI_BIAS : e == GELU ? IFX_EPI_GELU_TANH : e == RESIDUAL ? IFX_EPI_RESIDUAL : IFX_EPI_GATE_RES;
  if (e >= RESIDUAL) epi.residual = at(1024 + (op == RES8 ? 8 : 0)), epi.ld_res = N;
  if (e >= GATE1560) epi.mod = at(1280), epi.mod_slots = 6, epi.gate_slot = 2, epi.rows_per_group = e == GATE1560 ? 1560 : e == GATE40 ? 40 : 100;
  return epi;
}

// ws: 0 none, 1 what the query returned, 2 unlimited
static void bf16_call(int M, int N, int K, int e, int op, int ws, int y2 = 0) {
  ifx_epilogue epi = epilogue(e, op, N);
  if (y2) epi.y2 = at(1536), epi.ldy2 = N, epi.split_col = N >= 512 ? 256 : 0;
  const int64_t bytes = ws == 0 ? 0 : ws == 1 ? ifx_gemm_workspace_bytes(M, N, K) : (int64_t)1 << 40;
  begin();
  end(ifx_gemm_bf16_ws(at(0), K, at(256), at(768 + (op == BIAS4 ? 4 : 0)), at(512), op == LDY4 ? N + 4 : N, M, N, K, &epi,
                       ws == 0 ? nullptr : at(2048), bytes, nullptr));
}
static void q8_call(int M, int N, int K, int format, int e, int op, int ws) {
  const ifx_epilogue epi = epilogue(e, op, N);
  const int64_t bytes = ws == 0 ? 0 : ws == 1 ? ifx_gemm_q8_workspace_bytes(M, N, K) : (int64_t)1 << 40;
  begin();
  end(ifx_gemm_q8_ws(at(0), K, (const float*)at(1792), at(256), (const float*)at(1856), at(768 + (op == BIAS4 ? 4 : 0)), at(512),
                     op == LDY4 ? N + 4 : N, M, N, K, format, &epi, ws == 0 ? nullptr : at(2048), bytes, nullptr));
}
static void q8_quant_out_call(int M, int N, int K, int format) {
  const ifx_epilogue epi = epilogue(GELU, IDEAL, N);
  begin();
  end(ifx_gemm_q8_quant_out(at(0), K, (const float*)at(1792), at(256), (const float*)at(1856), at(768), at(512), N, M, N, K, format,
                            &epi, (const float*)at(1920), 0, nullptr));
}

int main() {
  static const int Ms[] = {0, 1, 64, 333, 512, 585, 1023, 1024, 1170, 1519, 2047, 2048, 2340, 4680, 6075, 9360, 10800, 12150, 43700, 70000};
  static const int NK[][2] = {{1536, 1536}, {4608, 1536}, {8960, 1536}, {1536, 8960}, {3072, 3072},  {8192, 3072}, {12288, 3072},
                              {3072, 12288}, {20480, 4096}, {4096, 10240}, {704, 4096}, {704, 256},   {712, 4096},  {1544, 1536},
                              {1540, 1536}, {2048, 4096}, {2048, 4160}, {6144, 6144}, {64, 64}};
  for (g_small_split = 0; g_small_split <= 1; ++g_small_split)
    for (g_variant = 0; g_variant <= 29; ++g_variant) {
      g_sum = 14695981039346656037ull, g_calls = 0;
      for (const int M : Ms)
        for (const auto& nk : NK) {
          const int N = nk[0], K = nk[1];
          fold(std::to_string(ifx_gemm_workspace_bytes(M, N, K)));
          for (int e = 0; e < N_EPI; ++e) {
            for (int ws = 0; ws <= 2; ++ws) bf16_call(M, N, K, e, IDEAL, ws);
            for (int op = LDY4; op < N_OPERANDS; ++op) bf16_call(M, N, K, e, op, 2);
          }
          for (int ws = 0; ws <= 2; ++ws) bf16_call(M, N, K, BIAS, IDEAL, ws, 1);     // y2 on the epilogue that carries it
          bf16_call(M, N, K, BIAS, LDY4, 2, 1);                                       // ... on operands the ping-pong tiles refuse
          bf16_call(M, N, K, RESIDUAL, IDEAL, 2, 1);                                  // ... and on one that does not: refused
        }
      printf("small_split %d variant %2d bf16: %6d calls, checksum %016llx\n", g_small_split, g_variant, g_calls, g_sum);
      g_sum = 14695981039346656037ull, g_calls = 0;
      for (const int M : Ms)
        for (const auto& nk : NK) {
          const int N = nk[0], K = nk[1];
          fold(std::to_string(ifx_gemm_q8_workspace_bytes(M, N, K)));
          if (K % 128 != 0) continue;
          for (const int format : {IFX_Q_FP8_E4M3, IFX_Q_INT8}) {
            for (int e = 0; e < N_EPI; ++e) {
              for (int ws = 0; ws <= 2; ++ws) q8_call(M, N, K, format, e, IDEAL, ws);
              for (int op = LDY4; op < N_OPERANDS; ++op) q8_call(M, N, K, format, e, op, 2);
            }
            q8_quant_out_call(M, N, K, format);
          }
        }
      printf("small_split %d variant %2d q8:   %6d calls, checksum %016llx\n", g_small_split, g_variant, g_calls, g_sum);
    }

  // the project's named shapes under the automatic choice, in full
  g_variant = 0;
  static const int block[4][2] = {{4608, 1536}, {1536, 1536}, {8960, 1536}, {1536, 8960}};
  static const int named[][4] = {{0, 4680, -1, 0}, {0, 10800, -1, 0}, {1, 585, -1, 0},         {1, 1170, -1, 0},        {1, 2340, -1, 0},
                                 {0, 1519, 8192, 3072}, {0, 1519, 12288, 3072}, {0, 512, 20480, 4096}};   // small_split, M, N or -1 = the block's four, K
  for (const auto& s : named)
    for (int b = 0; b < (s[2] < 0 ? 4 : 1); ++b) {
      g_small_split = s[0];
      const int M = s[1], N = s[2] < 0 ? block[b][0] : s[2], K = s[2] < 0 ? block[b][1] : s[3];
      for (const int e : {BIAS, GATE1560})
        for (int ws = 0; ws <= 1; ++ws) {
          bf16_call(M, N, K, e, IDEAL, ws);
          printf("small_split %d bf16 %5d x %5d x %5d %-9s workspace %-10s: %s\n", s[0], M, N, K, kEpiName[e],
                 ws ? std::to_string(ifx_gemm_workspace_bytes(M, N, K)).c_str() : "none", g_last.c_str());
        }
      q8_call(M, N, K, IFX_Q_FP8_E4M3, BIAS, IDEAL, 1);
      printf("small_split %d fp8  %5d x %5d x %5d %-9s workspace %-10s: %s\n", s[0], M, N, K, kEpiName[BIAS],
             std::to_string(ifx_gemm_q8_workspace_bytes(M, N, K)).c_str(), g_last.c_str());
    }
  return 0;
}

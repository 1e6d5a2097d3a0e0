// The host side of the LDS-DMA GEMM tiles (ifx::launch_gemm_lds_dma of inferix_amd/csrc/ifx_gemm_glds.hip) as a stand-alone host
// program, in the style of gemm_plan_check.cpp: which kernel instantiation a tile id launches, on which grid, with how many threads and
// how much dynamic LDS, and what it refuses — without a GPU and under the host sanitizers:
//   make -C inferix_amd/csrc plan_check        (hipcc ... -Xarch_host -fsanitize=address,undefined; builds and runs it)
// Every tile id 0 - 19 and one id without a name, over one-tile, ragged, "tiles per XCD do not divide" and "K/64 not a multiple of the
// K-groups" shapes and the four epilogues; every launch is recorded instead of made, one line per call:
//   a launch   : `<kernel instantiation> grid block lds`       (the four-wave register-staged tile of another file: `w4 splits`)
//   a refusal  : `rc <code> <the error text>`
// tests/test_cabi_and_host.py compares the output with what this program printed before the five launchers became one.
#include <stdarg.h>

#include <string>

#include "../inferix_amd/csrc/ifx_gemm_glds.hip"
#include "check_stubs.h"

static std::string g_launch, g_error;

extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  const std::string name = kernel_name(f);
  char b[64];
  snprintf(b, sizeof b, " %u %u %zu", grid.x, block.x, lds);
  g_launch += (g_launch.empty() ? "" : " + ") + name + b;
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetDeviceCount(int* n) { return *n = 1, hipSuccess; }      // one device: the launch path never asks which

namespace ifx {   // what the library's other files provide
void set_error(const char* fmt, ...) {
  char b[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_error = b;
}
int launch_gemm_w4(const unsigned short*, int, const unsigned short*, unsigned short*, int, int, int, int, int, const EpiArgs&,
                   hipStream_t, int splits, void* workspace) {
  g_launch += "w4 " + std::to_string(splits) + (workspace ? " WORKSPACE" : "");
  return IFX_OK;
}
}  // namespace ifx

alignas(64) static unsigned char g_mem[1024];   // operand addresses only: no launch is made, nothing is read or written
static unsigned short* at(int off) { return (unsigned short*)(g_mem + off); }

static void call(int tile, int M, int N, int K, int mode) {
  ifx::EpiArgs ea;
  ea.bias = at(768), ea.residual = at(512), ea.ld_res = N, ea.mod = at(640), ea.mod_slots = 6, ea.gate_slot = 2, ea.rows_per_group = 40;
  g_launch.clear(), g_error.clear();
  const int rc = ifx::launch_gemm_lds_dma(tile, at(0), K, at(128), at(256), N, M, N, K, mode, ea, nullptr);
  printf("tile %2d %5d x %5d x %5d epilogue %d: %s\n", tile, M, N, K, mode,
         rc != IFX_OK ? ("rc " + std::to_string(rc) + " " + g_error).c_str() : g_launch.empty() ? "no launch" : g_launch.c_str());
}

int main() {
  // one tile; ragged edges; two block shapes whose tile counts the eight XCDs do not divide on most tiles (the grid is rounded up);
  // K/64 = 6 (the four K-groups refuse) and 3 (the two refuse as well)
  static const int shapes[][3] = {{64, 64, 256}, {333, 712, 1536}, {2340, 1536, 1536}, {4680, 4608, 1536}, {585, 1536, 384}, {130, 264, 192}};
  static const int tiles[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 25};
  for (const int tile : tiles) {
    for (const auto& s : shapes) call(tile, s[0], s[1], s[2], IFX_EPI_BIAS);
    for (const int mode : {(int)IFX_EPI_GELU_TANH, (int)IFX_EPI_RESIDUAL, (int)IFX_EPI_GATE_RES, 99}) call(tile, 333, 712, 1536, mode);
  }
  return 0;
}

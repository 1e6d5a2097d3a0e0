// The host side of inferix_amd/csrc/ifx_conv.hip (ifx_conv3d_cl, ifx_rmsnorm_cl, ifx_softmax_rows) as a stand-alone host program, in the
// style of gemm_tile_launch_check.cpp: which kernel instantiation a call launches, on which grid, with how many threads and how much
// dynamic LDS, and what it refuses — without a GPU and under the host sanitizers:
//   make -C inferix_amd/csrc plan_check        (hipcc ... -Xarch_host -fsanitize=address,undefined; builds and runs it)
// The runtime is stubbed: a launch is recorded instead of made, nothing is allocated, read or written (only the descriptor's numbers
// matter, so a 2048 x 2048 frame costs nothing), and the current device is a fake index with its own CU count.  Every call gives
//   a launch   : `<kernel instantiation> grid block lds`
//   a refusal  : `rc <code> <the error text>`
// and calls that differ only in what cannot change the instantiation (in_planar; the number of output frames; the CU count, which sizes
// the persistent grid) share a line when they agree on kernel, block and LDS: `*` stands for the grid, and the nine grids follow as
// `t<t_out> <on 256 CUs>/<on 304>/<on 64>`.
// tests/test_cabi_and_host.py compares the output with what this program printed before the decisions moved into ifx_conv_plan.h (the
// lines of the alignment contract were added with it, later).
#include <stdarg.h>

#include <string>

#include "../inferix_amd/csrc/ifx_conv.hip"
#include "check_stubs.h"

struct Launch {
  std::string kernel;
  unsigned grid = 0, block = 0;
  size_t lds = 0;
  int n = 0;      // launches seen since the last reset
};
static Launch g_launch;
static std::string g_error;
static int g_dev = 0, g_variant = 0;
static const int kCus[3] = {256, 304, 64};      // fake devices 0, 1, 2

extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  const std::string name = kernel_name(f);
  g_launch.kernel = name, g_launch.grid = grid.x, g_launch.block = block.x, g_launch.lds = lds, ++g_launch.n;
  if (grid.y != 1 || grid.z != 1 || block.y != 1 || block.z != 1) g_launch.kernel += " (not one-dimensional)";
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetDeviceCount(int* n) { return *n = 3, hipSuccess; }      // more than one: the current device is asked for
extern "C" hipError_t hipGetDevice(int* dev) { return *dev = g_dev, hipSuccess; }
extern "C" hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int dev) { return *v = kCus[dev], hipSuccess; }

namespace ifx {   // what the library's other files provide
void set_error(const char* fmt, ...) {
  char b[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  g_error = b;
}
int conv_variant() { return g_variant; }
}  // namespace ifx

alignas(64) static unsigned char g_mem[2048];   // operand addresses only: no launch is made, nothing is read or written
static unsigned short* at(int off) { return (unsigned short*)(g_mem + off); }
static const int32_t kSlots[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// what a call did, as text: the kernel with block and LDS (or the refusal), and the grid apart
struct Outcome {
  std::string what, grid;
};
template <class Call>
static Outcome run(Call&& call) {
  g_launch = Launch(), g_error.clear();
  const int rc = call();
  if (rc != IFX_OK) return {"rc " + std::to_string(rc) + " " + g_error, ""};
  if (g_launch.n != 1) return {std::to_string(g_launch.n) + " launches", ""};
  return {g_launch.kernel + " GRID " + std::to_string(g_launch.block) + " " + std::to_string(g_launch.lds), std::to_string(g_launch.grid)};
}
static std::string line(const Outcome& o, const std::string& grid) {      // `<kernel> grid block lds`
  std::string s = o.what;
  const size_t p = s.find(" GRID ");
  return p == std::string::npos ? s : s.replace(p + 1, 4, grid);
}
static std::string line(const Outcome& o) { return line(o, o.grid); }

static ifx_conv3d_desc conv_desc(int hs, int ws, int cin, int cout, int kt, int ks, int upsample, int t_out, int planar) {
  ifx_conv3d_desc d = {};
  d.x = at(0), d.w = at(256), d.bias = at(512), d.y = at(768), d.zero_page = at(1024);
  d.in_slots = d.out_slots = kSlots;
  d.in_frame_stride = (int64_t)hs * ws * cin, d.out_frame_stride = ((int64_t)hs * ws * cout) << (2 * upsample);
  d.hs = hs, d.ws = ws, d.cin = cin, d.cout = cout, d.kt = kt, d.ks = ks, d.t_out = t_out, d.upsample = upsample, d.in_planar = planar;
  return d;
}
static Outcome conv_call(const ifx_conv3d_desc& d, int variant = 0, int dev = 0) {
  g_variant = variant, g_dev = dev;
  return run([&] { return ifx_conv3d_cl(&d, nullptr); });
}
static void conv_line(const char* label, const ifx_conv3d_desc& d, int variant = 0) {
  printf("conv %s: %s\n", label, line(conv_call(d, variant)).c_str());
}

// one (cout, kernel shape, kt, variant, frame): in_planar 0 / 1 x three t_out x three CU counts
static void conv_group(int cout, int ks, int ups, int kt, int variant, int hs, int ws) {
  const int t_outs[3] = {1, 3, ifx::conv::MAXF - kt + 1};
  Outcome o[2][3][3];
  bool same = true;
  for (int pl = 0; pl < 2; ++pl)
    for (int t = 0; t < 3; ++t)
      for (int c = 0; c < 3; ++c) {
        o[pl][t][c] = conv_call(conv_desc(hs, ws, 64, cout, kt, ks, ups, t_outs[t], pl), variant, c);
        same = same && o[pl][t][c].what == o[0][0][0].what && !o[pl][t][c].grid.empty() && o[pl][t][c].grid == o[0][t][c].grid;
      }
  char head[96];
  snprintf(head, sizeof head, "conv cout %3d ks %d ups %d kt %d variant %d %2dx%-3d", cout, ks, ups, kt, variant, hs, ws);
  if (same) {
    std::string grids;
    for (int t = 0; t < 3; ++t)
      grids += " t" + std::to_string(t_outs[t]) + " " + o[0][t][0].grid + "/" + o[0][t][1].grid + "/" + o[0][t][2].grid;
    printf("%s: %s grids%s\n", head, line(o[0][0][0], "*").c_str(), grids.c_str());
    return;
  }
  for (int pl = 0; pl < 2; ++pl)
    for (int t = 0; t < 3; ++t)
      for (int c = 0; c < 3; ++c)
        printf("%s planar %d t_out %d cus %d: %s\n", head, pl, t_outs[t], kCus[c], line(o[pl][t][c]).c_str());
}

static Outcome norm_call(const void* x, const void* gamma, void* y, const int32_t* slots, int frames, int frame_pixels, int channels, int flags) {
  return run([&] {
    return ifx_rmsnorm_cl((const ifx_bf16*)x, (const ifx_bf16*)gamma, (ifx_bf16*)y, (int64_t)frame_pixels * channels, slots, frames, frame_pixels,
                          channels, flags, nullptr);
  });
}
static void norm_line(const char* label, const Outcome& o) { printf("norm %s: %s\n", label, line(o).c_str()); }

int main() {
  // ---- ifx_conv3d_cl: every channel-tile choice, kernel shape, kernel choice and grid
  static const int couts[] = {3, 16, 24, 32, 48, 64, 96, 128, 160, 192, 288, 384, 512, 576, 640};
  static const int shapes[][2] = {{1, 0}, {3, 0}, {3, 1}};      // (ks, upsample)
  static const int frames[][2] = {{8, 64}, {13, 70}, {60, 104}};
  for (const int cout : couts)
    for (const auto& sh : shapes)
      for (const int kt : {1, 3})
        for (const int variant : {0, 1})
          for (const auto& f : frames) conv_group(cout, sh[0], sh[1], kt, variant, f[0], f[1]);
  // the three "operand of 2 GiB or more -> lock-step kernel" clauses, just under and just over
  conv_line("input 2048x2047 cin 256 cout 96 (under 2 GiB)", conv_desc(2048, 2047, 256, 96, 3, 3, 0, 1, 0));
  conv_line("input 2048x2048 cin 256 cout 96 (2 GiB)", conv_desc(2048, 2048, 256, 96, 3, 3, 0, 1, 0));
  conv_line("output 2048x1365 cin 32 cout 384 (under 2 GiB)", conv_desc(2048, 1365, 32, 384, 3, 3, 0, 1, 0));
  conv_line("output 2048x1366 cin 32 cout 384 (over 2 GiB)", conv_desc(2048, 1366, 32, 384, 3, 3, 0, 1, 0));
  conv_line("output 1024x682 upsampled cin 32 cout 384 (under 2 GiB)", conv_desc(1024, 682, 32, 384, 1, 3, 1, 1, 0));
  conv_line("output 1024x683 upsampled cin 32 cout 384 (over 2 GiB)", conv_desc(1024, 683, 32, 384, 1, 3, 1, 1, 0));
  conv_line("weights kt 3 cin 82848 cout 480 (under 2 GiB)", conv_desc(8, 64, 82848, 480, 3, 3, 0, 1, 0));
  conv_line("weights kt 3 cin 82880 cout 480 (over 2 GiB)", conv_desc(8, 64, 82880, 480, 3, 3, 0, 1, 0));
  conv_line("weights kt 1 cin 82880 cout 480", conv_desc(8, 64, 82880, 480, 1, 3, 0, 1, 0));
  // every refusal of the entry point
  {
    g_variant = 0, g_dev = 0;
    printf("conv null descriptor: %s\n", line(run([] { return ifx_conv3d_cl(nullptr, nullptr); })).c_str());
    const ifx_conv3d_desc ok = conv_desc(8, 64, 32, 96, 3, 3, 0, 1, 0);
    ifx_conv3d_desc d = ok;
    d.x = nullptr, conv_line("null x", d), d = ok;
    d.w = nullptr, conv_line("null w", d), d = ok;
    d.y = nullptr, conv_line("null y", d), d = ok;
    d.zero_page = nullptr, conv_line("null zero page", d), d = ok;
    d.bias = nullptr, conv_line("no bias", d), d = ok;
    d.kt = 2, conv_line("kt 2", d), d = ok;
    d.ks = 2, conv_line("ks 2", d), d = ok;
    d.ks = 1, d.upsample = 1, conv_line("upsample with ks 1", d), d = ok;
    d.upsample = 2, conv_line("upsample 2", d), d = ok;
    d.cin = 0, conv_line("cin 0", d), d = ok;
    d.cin = 48, conv_line("cin 48", d), d = ok;
    d.in_planar = 2, conv_line("in_planar 2", d), d = ok;
    d.cout = 0, conv_line("cout 0", d), d = ok;
    d.cout = 6, conv_line("cout 6", d), d = ok;
    d.cout = 2, conv_line("cout 2", d), d = ok;
    d.t_out = 0, conv_line("t_out 0", d), d = ok;
    d.t_out = 15, conv_line("t_out 15 with kt 3", d), d = ok;
    d.t_out = 16, d.kt = 1, conv_line("t_out 16 with kt 1", d), d = ok;
    d.t_out = 17, d.kt = 1, conv_line("t_out 17 with kt 1", d), d = ok;
    d.hs = 0, conv_line("hs 0", d), d = ok;
    d.ws = 0, conv_line("ws 0", d), d = ok;
    conv_line("input frame 4096x2048 cin 256", conv_desc(4096, 2048, 256, 96, 3, 3, 0, 1, 0));
    conv_line("output frame 4096x2048 cout 256", conv_desc(4096, 2048, 32, 256, 3, 3, 0, 1, 0));
    conv_line("upsampled output frame 2048x1024 cout 256", conv_desc(2048, 1024, 32, 256, 1, 3, 1, 1, 0));
    conv_line("upsampled output frame 2048x1023 cout 256", conv_desc(2048, 1023, 32, 256, 1, 3, 1, 1, 0));
    // the alignment contract: 16-byte moves from x and w always, to y and from residual when cout % 8 == 0
    d.in_frame_stride += 4, conv_line("in_frame_stride + 4", d), d = ok;
    d.in_frame_stride += 64, d.out_frame_stride += 64, conv_line("frame strides + 64", d), d = ok;
    d.x = at(8), conv_line("x + 8 bytes", d), d = ok;
    d.w = at(256 + 2), conv_line("w + 2 bytes", d), d = ok;
    d.out_frame_stride += 4, conv_line("out_frame_stride + 4", d), d = ok;
    d.y = at(768 + 8), conv_line("y + 8 bytes", d), d = ok;
    d.residual = at(1280), conv_line("residual", d), d = ok;
    d.residual = at(1280 + 8), conv_line("residual + 8 bytes", d), d = ok;
    d.cout = 20, d.out_frame_stride = 8 * 64 * 20 + 4, d.y = at(768 + 2), d.residual = at(1280 + 2), conv_line("cout 20: out_frame_stride + 4, y and residual + 2 bytes", d), d = ok;
    d.cout = 20, d.in_frame_stride += 4, conv_line("cout 20: in_frame_stride + 4", d), d = ok;
  }

  // ---- ifx_rmsnorm_cl: the instantiation of every channel count, and its block count for 1, 4095 and 3 x 60 x 104 pixels
  for (int ch = 8; ch <= 512; ch += 8) {
    const Outcome o[3] = {norm_call(at(0), at(256), at(512), kSlots, 1, 1, ch, 0), norm_call(at(0), at(256), at(512), kSlots, 1, 4095, ch, IFX_NORM_SILU),
                          norm_call(at(0), at(256), at(512), kSlots, 3, 60 * 104, ch, ch % 32 == 0 ? IFX_NORM_SILU | IFX_NORM_OUT_PLANAR : 0)};
    if (o[1].what == o[0].what && o[2].what == o[0].what && !o[0].grid.empty())
      printf("norm channels %3d: %s grids %s/%s/%s\n", ch, line(o[0], "*").c_str(), o[0].grid.c_str(), o[1].grid.c_str(), o[2].grid.c_str());
    else
      for (const Outcome& x : o) printf("norm channels %3d: %s\n", ch, line(x).c_str());
  }
  norm_line("null x", norm_call(nullptr, at(256), at(512), kSlots, 1, 64, 96, 0));
  norm_line("null gamma", norm_call(at(0), nullptr, at(512), kSlots, 1, 64, 96, 0));
  norm_line("null y", norm_call(at(0), at(256), nullptr, kSlots, 1, 64, 96, 0));
  norm_line("null slots", norm_call(at(0), at(256), at(512), nullptr, 1, 64, 96, 0));
  norm_line("frames 0", norm_call(at(0), at(256), at(512), kSlots, 0, 64, 96, 0));
  norm_line("frames 16", norm_call(at(0), at(256), at(512), kSlots, 16, 64, 96, 0));
  norm_line("frames 17", norm_call(at(0), at(256), at(512), kSlots, 17, 64, 96, 0));
  norm_line("frame_pixels 0", norm_call(at(0), at(256), at(512), kSlots, 1, 0, 96, 0));
  norm_line("16 x 134213632 pixels", norm_call(at(0), at(256), at(512), kSlots, 16, 134213632, 96, 0));
  norm_line("16 x 134213631 pixels", norm_call(at(0), at(256), at(512), kSlots, 16, 134213631, 96, 0));
  norm_line("channels 0", norm_call(at(0), at(256), at(512), kSlots, 1, 64, 0, 0));
  norm_line("channels 12", norm_call(at(0), at(256), at(512), kSlots, 1, 64, 12, 0));
  norm_line("channels 520", norm_call(at(0), at(256), at(512), kSlots, 1, 64, 520, 0));
  norm_line("flags 4", norm_call(at(0), at(256), at(512), kSlots, 1, 64, 96, 4));
  norm_line("planar with channels 72", norm_call(at(0), at(256), at(512), kSlots, 1, 64, 72, IFX_NORM_OUT_PLANAR));

  // ---- ifx_softmax_rows
  printf("softmax 6240 x 6240: %s\n", line(run([] { return ifx_softmax_rows((const ifx_bf16*)at(0), (ifx_bf16*)at(256), 6240, 6240, 6240, 0.05f, nullptr); })).c_str());
  printf("softmax 5 x 70 ld 72: %s\n", line(run([] { return ifx_softmax_rows((const ifx_bf16*)at(0), (ifx_bf16*)at(256), 5, 70, 72, 1.f, nullptr); })).c_str());
  printf("softmax ld 70: %s\n", line(run([] { return ifx_softmax_rows((const ifx_bf16*)at(0), (ifx_bf16*)at(256), 5, 70, 70, 1.f, nullptr); })).c_str());
  return 0;
}

// The launch mechanics of inferix_amd/csrc/ifx_launch.h (dynamic-LDS opt-in per kernel and device, checked, from any number of host
// threads; CU count per device) as a stand-alone host program, so that they can run without a GPU, on fake devices, under the host
// sanitizers and without loading the library into another process:
//   make -C inferix_amd/csrc plan_check        (builds and runs it under ASan + UBSan, then under TSan)
// It includes the real ifx_conv.hip and ifx_t5.hip and drives ifx_conv3d_cl (lock-step and persistent kernel, with and without
// upsample) and ifx_t5_attention.  What the other files provide is stubbed, and so is the runtime: the current device is a fake index
// of the calling thread, every fake device has its own CU count, an opt-in can be refused on one device, and a launch is recorded as
// (kernel, device, grid) instead of made.  Exits 0 when every rule holds, else prints the broken ones and exits 1.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../inferix_amd/csrc/ifx_conv.hip"
#include "../inferix_amd/csrc/ifx_t5.hip"
#include "check_stubs.h"

// ---- the fake runtime --------------------------------------------------------------------------------------------------------------
static thread_local int t_dev = 0;               // the calling thread's current device
static thread_local bool t_no_device = false;    // hipGetDevice fails
static thread_local int t_variant = 0;           // conv_variant
static thread_local char t_error[512];
static std::atomic<int> g_refuse_on{-1};         // the opt-in is refused on this device
static std::atomic<bool> g_no_cu_count{false};   // the CU query fails
static int cus_of(int dev) { return dev == 1 ? 64 : dev == 2 ? 128 : dev == 3 ? 304 : 256; }

struct Seen {
  int requests = 0, launches = 0, early = 0;     // successful opt-ins; launches; launches with no successful opt-in before them
  unsigned grid = 0;                             // of the last launch
};
static std::mutex g_mu;
static std::map<std::pair<const void*, int>, Seen> g_seen;             // (kernel, device; -1 = unknown)
static std::map<std::pair<int, std::thread::id>, int> g_cu_queries;   // (device, thread)
static int seen_dev() { return t_no_device ? -1 : t_dev; }

extern "C" hipError_t hipGetDeviceCount(int* n) { return *n = 128, hipSuccess; }      // more than one: the current device is asked for
extern "C" hipError_t hipGetDevice(int* dev) {
  if (t_no_device) return hipErrorNoDevice;
  return *dev = t_dev, hipSuccess;
}
extern "C" hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int dev) {
  std::lock_guard<std::mutex> lock(g_mu);
  ++g_cu_queries[{dev, std::this_thread::get_id()}];
  if (g_no_cu_count) return hipErrorInvalidDevice;
  return *v = cus_of(dev), hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int) {
  if (!t_no_device && g_refuse_on == t_dev) return hipErrorInvalidValue;
  std::lock_guard<std::mutex> lock(g_mu);
  ++g_seen[{f, seen_dev()}].requests;
  return hipSuccess;
}
extern "C" hipError_t hipGetLastError() { return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "refused by the fake runtime"; }
extern "C" hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3, void**, size_t, hipStream_t) {
  std::lock_guard<std::mutex> lock(g_mu);
  Seen& s = g_seen[{f, seen_dev()}];
  ++s.launches, s.grid = grid.x;
  if (s.requests == 0) ++s.early;
  return hipSuccess;
}

namespace ifx {   // what the library's other files provide
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_error, sizeof(t_error), fmt, ap);
  va_end(ap);
}
int conv_variant() { return t_variant; }
}  // namespace ifx

// ---- the calls ---------------------------------------------------------------------------------------------------------------------
alignas(64) static unsigned char g_mem[4096];   // operand addresses only: no launch is made, nothing is read or written
static unsigned short* at(int off) { return (unsigned short*)(g_mem + off); }
static const int32_t kSlots[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// 3 x 3 x 3, 32 -> 96 channels: the persistent kernel under conv_variant 0, the lock-step one under 1
static int conv_call(int hs, int ws, int t_out, int upsample, int variant) {
  ifx_conv3d_desc d = {};
  d.x = at(0), d.w = at(256), d.bias = at(512), d.y = at(768), d.zero_page = at(1024);
  d.in_slots = d.out_slots = kSlots;
  d.in_frame_stride = (int64_t)hs * ws * 32, d.out_frame_stride = ((int64_t)hs * ws * 96) << (2 * upsample);
  d.hs = hs, d.ws = ws, d.cin = 32, d.cout = 96, d.kt = 3, d.ks = 3, d.t_out = t_out, d.upsample = upsample;
  t_variant = variant;
  return ifx_conv3d_cl(&d, nullptr);
}
static int t5_call() {
  return ifx_t5_attention(at(0), 64, at(256), 64, at(512), 64, at(768), 64, at(1024), (const int32_t*)at(1280), 1, 128, 1, nullptr);
}
static int call(int i) { return i < 4 ? conv_call(8, 64, 1, i & 1, i >> 1) : t5_call(); }      // the five kernels behind the entry points
constexpr int kCalls = 5;

static int g_failed = 0;
#define EXPECT(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      printf("BROKEN (%s): ", #cond);        \
      printf(__VA_ARGS__);                   \
      printf("\n");                          \
      ++g_failed;                            \
    }                                        \
  } while (0)

// what was seen on `dev` since `before`, summed over the kernels
static Seen on_device(int dev, const std::map<std::pair<const void*, int>, Seen>& before = {}) {
  std::lock_guard<std::mutex> lock(g_mu);
  Seen sum;
  for (const auto& [key, s] : g_seen)
    if (key.second == dev) {
      const auto b = before.find(key);
      const Seen zero, &was = b == before.end() ? zero : b->second;
      sum.requests += s.requests - was.requests, sum.launches += s.launches - was.launches, sum.early += s.early - was.early;
      if (s.launches > was.launches) sum.grid = s.grid;
    }
  return sum;
}

int main() {
  // 1. eight threads over four devices, 1000 calls each: no launch of a kernel on a device before a successful opt-in for that pair,
  //    and at most one opt-in per thread on the device
  constexpr int kThreads = 8, kDevices = 4, kRounds = 200;
  {
    std::atomic<int> ready{0}, bad_rc{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; ++t)
      threads.emplace_back([&, t] {
        t_dev = t % kDevices;
        ++ready;
        while (ready < kThreads) std::this_thread::yield();
        for (int r = 0; r < kRounds; ++r)
          for (int i = 0; i < kCalls; ++i)
            if (call((i + t) % kCalls) != IFX_OK) ++bad_rc;
      });
    for (auto& th : threads) th.join();
    EXPECT(bad_rc == 0, "%d calls failed: %s", (int)bad_rc, t_error);
    EXPECT((int)g_seen.size() == kCalls * kDevices, "%zu (kernel, device) pairs launched, not %d", g_seen.size(), kCalls * kDevices);
    for (const auto& [key, s] : g_seen) {
      EXPECT(s.early == 0, "device %d: %d of %d launches of kernel %p had no opt-in before them", key.second, s.early, s.launches, key.first);
      EXPECT(s.requests >= 1 && s.requests <= kThreads / kDevices, "device %d kernel %p: %d opt-ins", key.second, key.first, s.requests);
      EXPECT(s.launches == kRounds * kThreads / kDevices, "device %d kernel %p: %d launches", key.second, key.first, s.launches);
    }
  }
  // 2. a refused opt-in: IFX_ELAUNCH, no launch, the entry point named; asked again, and launched, once the device grants it
  t_dev = 5, g_refuse_on = 5;
  for (int i = 0; i < kCalls; ++i) {
    t_error[0] = 0;
    EXPECT(call(i) == IFX_ELAUNCH, "call %d", i);
    EXPECT(strstr(t_error, i < 4 ? "ifx_conv3d_cl" : "ifx_t5_attention") && strstr(t_error, "refused by the fake runtime"), "call %d: \"%s\"", i, t_error);
  }
  EXPECT(on_device(5).launches == 0 && on_device(5).requests == 0, "launched on the refusing device");
  g_refuse_on = -1;
  for (int i = 0; i < kCalls; ++i) EXPECT(call(i) == IFX_OK, "call %d", i);
  EXPECT(on_device(5).requests == kCalls && on_device(5).launches == kCalls && on_device(5).early == 0, "after the refusal ended");
  // 3. no current device, or one past the cache: the opt-in goes in front of every launch
  for (const int dev : {-1, 70}) {
    t_no_device = dev < 0, t_dev = dev < 0 ? 0 : dev;
    for (int r = 0; r < 3; ++r)
      for (int i = 0; i < kCalls; ++i) EXPECT(call(i) == IFX_OK, "call %d", i);
    const Seen s = on_device(dev);
    EXPECT(s.requests == 3 * kCalls && s.launches == 3 * kCalls && s.early == 0, "device %d: %d opt-ins for %d launches", dev, s.requests, s.launches);
  }
  t_no_device = false;
  // 4. the persistent grid: min(CUs / 8, per_xcd) * 8 with the CUs of the calling thread's device.  Twelve upsampled frames of
  //    60 x 104 are 4 x 15 x 12 = 720 tiles, 90 per XCD
  for (const int dev : {0, 1, 2, 3}) {
    t_dev = dev;
    const auto before = g_seen;
    EXPECT(conv_call(60, 104, 12, 1, 0) == IFX_OK, "device %d", dev);
    const Seen s = on_device(dev, before);
    EXPECT(s.launches == 1 && s.grid == (unsigned)std::min(cus_of(dev) / 8, 90) * 8, "device %d (%d CUs): grid %u", dev, cus_of(dev), s.grid);
  }
  EXPECT(cus_of(0) == 256 && cus_of(1) == 64, "the grids above differ between a 256-CU and a 64-CU device");
  t_dev = 6, g_no_cu_count = true;      // the query fails: 256 CUs
  EXPECT(conv_call(60, 104, 12, 1, 0) == IFX_OK && on_device(6).grid == 32 * 8, "grid %u without a CU count", on_device(6).grid);
  g_no_cu_count = false;
  for (const auto& [key, n] : g_cu_queries)      // (a device past the cache is asked every time: 70 above)
    EXPECT(n <= 1 || key.first >= ifx::kLaunchDevices, "device %d: %d CU queries from one thread", key.first, n);
  EXPECT(!g_cu_queries.empty(), "no CU query seen");

  if (g_failed) return printf("launch_check: %d rules broken\n", g_failed), 1;
  printf("launch_check: %d threads x %d calls on %d devices, refusal, unknown device and persistent grids: all rules hold\n", kThreads,
         kRounds * kCalls, kDevices);
  return 0;
}

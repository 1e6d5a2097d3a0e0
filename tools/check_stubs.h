// What the stand-alone *_check.cpp programs share of their fake runtime; include it after the .hip files under test.
// kernel<<<...>>> = push the configuration, pop it in the kernel's host stub, hipLaunchKernel: the first two are here, the third is where a
// program records what it wants to see, so every program defines it itself — as it does the device queries it fakes and ifx::set_error.
#pragma once
#include <cxxabi.h>
#include <dlfcn.h>

#include <string>

static thread_local dim3 t_grid, t_block;      // (thread_local: launch_check.cpp launches from eight threads)
static thread_local size_t t_lds;
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t) {
  t_grid = grid, t_block = block, t_lds = lds;
  return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  *grid = t_grid, *block = t_block, *lds = t_lds, *stream = nullptr;
  return hipSuccess;
}

// the kernel instantiation behind the handle a launch passes, demangled, without its parameter list (link with -rdynamic -ldl)
static inline std::string kernel_name(const void* f) {
  Dl_info info;
  std::string name = "?";
  if (dladdr(f, &info) && info.dli_sname) {
    int st = 0;
    char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    name = st == 0 && d ? d : info.dli_sname;
    free(d);
    name = name.substr(0, name.find('('));
  }
  return name;
}

namespace ifx {
int check_launch(const char*) { return IFX_OK; }      // nothing was launched
}

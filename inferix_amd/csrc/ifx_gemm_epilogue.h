// The fused epilogues of the GEMM family (ifx_gemm.hip, ifx_gemm_glds.hip, ifx_gemm_w4.hip, ifx_gemm_pp.hip, ifx_quant.hip), ONCE:
// the kernel argument struct, the arithmetic on a vector of bf16 Linear outputs, the row store of the LDS-transposed epilogues, the
// mode -> instantiation switch, the ifx_epilogue -> kernel arguments translation, and the launcher prototypes of the family.
//
//   IFX_EPI_BIAS      : y = v                         v = bf16(acc + bias), the bf16 Linear output, in every epilogue
//   IFX_EPI_GELU_TANH : y = bf16(gelu(v))             tanh form, or the exact erf form under EpiArgs::gelu_erf()
//   IFX_EPI_RESIDUAL  : y = bf16(res + v)
//   IFX_EPI_GATE_RES  : y = bf16(res + bf16(v * gate[row / rows_per_group]))
//
// A new epilogue (or a changed rounding rule) is added here and nowhere else.
#pragma once
#include <type_traits>

#include "ifx_common.h"
#include "ifx_gemm_plan.h"
#include "ifx_launch.h"

namespace ifx {

struct EpiArgs {
  const unsigned short* bias = nullptr;
  const unsigned short* residual = nullptr;
  int ld_res = 0;
  const unsigned short* mod = nullptr;
  int mod_slots = 1, gate_slot = 0, rows_per_group = 1;
  // exact (erf) GELU as torch.nn.functional.gelu evaluates it on a bf16 tensor: fp32 math, one rounding (MAGI CustomMLP,
  // inferix/models/magi/dit/dit_module.py:552).  Selected at run time inside the GELU epilogue instantiation: the epilogue's
  // otherwise unused `gate_slot` field carries 1 for IFX_EPI_GELU_ERF (resolve_epilogue sets it, no extra kernel argument).
  __host__ __device__ bool gelu_erf() const { return gate_slot != 0; }
};

// 8-bit operands (ifx_gemm_q8*): per-token / per-channel dequantisation scales, and (GELU epilogues) an optional static quantiser of
// the result for the next linear (ifx_gemm_q8_quant_out): y then holds e4m3 bytes (ldy in bytes), q = div_clamp_to(bf16 result, qdiv[n])
struct EpiArgsQ : EpiArgs {
  const float* sa = nullptr;
  const float* sw = nullptr;
  const float* qdiv = nullptr;
  int q_via_bf16 = 0;
};

// the ping-pong tiles: + the second destination (ifx_epilogue.y2): column tiles from split_col on are stored to y2 (row stride ldy2)
// at column n - split_col
struct EpiArgsP : EpiArgsQ {
  unsigned short* y2 = nullptr;
  int ldy2 = 0, split_col = 0;
};

template <int W>
using u16v = unsigned short __attribute__((ext_vector_type(W)));

// W bf16 Linear outputs vv (+ residual values rv, gate values gv where the epilogue has them) -> W bf16 results
template <int EPI, int W>
__device__ __forceinline__ u16v<W> epi_combine(const u16v<W> vv, const u16v<W> rv, const u16v<W> gv, const bool erf) {
  u16v<W> o;
  if constexpr (EPI == IFX_EPI_BIAS) {
    o = vv;
  } else if constexpr (EPI == IFX_EPI_GELU_TANH) {
    if (erf) {   // a scalar branch around the loop, not a per-element select
#pragma unroll
      for (int e = 0; e < W; ++e) o[e] = f2bf(gelu_erf_f(bf2f(vv[e])));
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) o[e] = f2bf(gelu_tanh_fast(bf2f(vv[e])));
    }
  } else if constexpr (EPI == IFX_EPI_RESIDUAL) {
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = f2bf(bf2f(rv[e]) + bf2f(vv[e]));
  } else {
    static_assert(EPI == IFX_EPI_GATE_RES, "epilogue");
#pragma unroll
    for (int e = 0; e < W; ++e) o[e] = f2bf(bf2f(rv[e]) + rbf(bf2f(vv[e]) * bf2f(gv[e])));
  }
  return o;
}

// the same on W consecutive channels of token row m from channel n on: fetches the residual / gate values the epilogue needs
template <int EPI, int W>
__device__ __forceinline__ u16v<W> epi_apply(const u16v<W> vv, int m, int n, int N, const EpiArgs& ea) {
  u16v<W> rv = vv, gv = vv;
  if constexpr (EPI == IFX_EPI_RESIDUAL || EPI == IFX_EPI_GATE_RES)
    rv = *reinterpret_cast<const u16v<W>*>(ea.residual + (size_t)m * ea.ld_res + n);
  if constexpr (EPI == IFX_EPI_GATE_RES)
    gv = *reinterpret_cast<const u16v<W>*>(ea.mod + ((size_t)(m / ea.rows_per_group) * ea.mod_slots + ea.gate_slot) * N + n);
  return epi_combine<EPI, W>(vv, rv, gv, ea.gelu_erf());
}

// the row store of the LDS-transposed epilogues: 8 channels (16 bytes) of one token; the caller has tested m < M and n < N
template <int EPI>
__device__ __forceinline__ void epi_store_row(const u16x8 vv, int m, int n, int N, const EpiArgs& ea, unsigned short* __restrict__ y,
                                              int ldy) {
  *reinterpret_cast<u16x8*>(y + (size_t)m * ldy + n) = epi_apply<EPI, 8>(vv, m, n, N, ea);
}

// host side -------------------------------------------------------------------------------------------------------------------------

// mode -> launch(std::integral_constant<int, IFX_EPI_*>), whose return code it hands on; `what` names the caller in the error text of an unknown mode
template <typename F>
static inline int dispatch_epilogue(int mode, const char* what, F&& launch) {
  switch (mode) {
    case IFX_EPI_BIAS: return launch(std::integral_constant<int, IFX_EPI_BIAS>{});
    case IFX_EPI_GELU_TANH: return launch(std::integral_constant<int, IFX_EPI_GELU_TANH>{});
    case IFX_EPI_RESIDUAL: return launch(std::integral_constant<int, IFX_EPI_RESIDUAL>{});
    case IFX_EPI_GATE_RES: return launch(std::integral_constant<int, IFX_EPI_GATE_RES>{});
    default: set_error("%s: unknown epilogue %d", what, mode); return IFX_EINVAL;
  }
}

// ifx_epilogue (may be null: bias only) -> the instantiation `mode` and the common kernel arguments; `who` = the entry point's name
static inline int resolve_epilogue(const ifx_epilogue* epi, const unsigned short* bias, const char* who, int* mode, EpiArgs* ea) {
  *mode = epi ? epi->epilogue : IFX_EPI_BIAS;
  *ea = EpiArgs{};
  ea->bias = bias;
  if (*mode == IFX_EPI_GELU_ERF) {       // the GELU instantiation with the exact-erf activation selected at run time
    *mode = IFX_EPI_GELU_TANH;
    ea->gate_slot = 1;
  }
  if (*mode == IFX_EPI_RESIDUAL || *mode == IFX_EPI_GATE_RES) {
    IFX_REQUIRE(epi->residual && epi->ld_res % 4 == 0, "%s: residual epilogue needs residual/ld_res", who);
    ea->residual = epi->residual;
    ea->ld_res = epi->ld_res;
  }
  if (*mode == IFX_EPI_GATE_RES) {
    IFX_REQUIRE(epi->mod && epi->rows_per_group > 0 && epi->gate_slot >= 0 && epi->gate_slot < epi->mod_slots,
                "%s: gate epilogue needs mod/mod_slots/gate_slot/rows_per_group", who);
    ea->mod = epi->mod;
    ea->mod_slots = epi->mod_slots;
    ea->gate_slot = epi->gate_slot;
    ea->rows_per_group = epi->rows_per_group;
  }
  return IFX_OK;
}

// what the ping-pong tiles ask about an epilogue's operands, for pp_epilogue_fits (ifx_gemm_plan.h)
static inline PpOperands pp_operands(const EpiArgs& ea) {
  return {!((uintptr_t)ea.bias & 7), !((uintptr_t)ea.residual & 15) && ea.ld_res % 8 == 0, !((uintptr_t)ea.mod & 15), ea.rows_per_group};
}

// what gemm_plan / gemm_q8_plan may see of a call with the resolved epilogue `mode` / `ea`; `workspace` may be null
static inline GemmRequest gemm_request(int M, int N, int K, int mode, const EpiArgs& ea, const void* y, int ldy, const void* workspace,
                                       int64_t workspace_bytes) {
  GemmRequest r;
  r.M = M, r.N = N, r.K = K, r.mode = mode;
  r.wide_ok = N % 8 == 0 && ldy % 8 == 0 && (ea.residual == nullptr || ea.ld_res % 8 == 0) &&
              !(((uintptr_t)y | (uintptr_t)ea.residual | (uintptr_t)ea.mod) & 15);
  r.ops = pp_operands(ea);
  r.ws_bytes = workspace != nullptr ? workspace_bytes : 0;
  return r;
}

// launchers ---------------------------------------------------------------------------------------------------------------------------
// what to launch, on which tile and with which K split is decided by gemm_plan / gemm_q8_plan (ifx_gemm_plan.h)
// LDS-DMA tiles (ifx_gemm_glds.hip): `tile` is a GemmTile
int launch_gemm_lds_dma(int tile, const unsigned short* x, int ldx, const unsigned short* w, unsigned short* y, int ldy, int M, int N,
                        int K, int mode, const EpiArgs& ea, hipStream_t s);
// four-wave 256 x 256 tile (ifx_gemm_w4.hip); splits == 2 needs gemm_w4_workspace_bytes(M, N, 2) bytes of workspace
int launch_gemm_w4(const unsigned short* x, int ldx, const unsigned short* w, unsigned short* y, int ldy, int M, int N, int K,
                   int mode, const EpiArgs& ea, hipStream_t s, int splits, void* workspace);
// persistent ping-pong tiles (ifx_gemm_pp.hip): 64 tj tokens x 256 channels; ks as in GemmPlan (0 stream-K, 1 unsplit, 2 / 4 / 8 K
// parts), `workspace` is read only when ks != 1; ea.sa != nullptr: 8-bit operands (x / w point at bytes), e4m3 or (q8_int8) int8
int launch_gemm_pp(const unsigned short* x, int ldx, const unsigned short* w, unsigned short* y, int ldy, int M, int N, int K,
                   int mode, const EpiArgsP& ea, hipStream_t s, int tj, int ks, void* workspace, int q8_int8 = 0);

}  // namespace ifx

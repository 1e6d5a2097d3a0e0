// The glue between the forwards of a guided many-step sampler (CausalDiffusionInferencePipeline: FlowUniPCMultistepScheduler.step,
// models/wan_base/utils/fm_solvers_unipc.py:655-739, behind the classifier-free-guidance mix of the pipeline's step loop) in ONE launch.
// Every coefficient of a UniPC step is a function of the sigma schedule alone, so the step is a linear form of six tensors with
// host-known scalars (inferix_amd/schedulers.py FlowUniPCSchedule.coefficients):
//   flow   = flow_uncond + guidance (flow_cond - flow_uncond)
//   m_t    = x - sigma flow                                                             (the x0 prediction; output 3)
//   x_c    = c_last last + c_m1 m1 + c_d1 (m2 - m1) + c_dt (m_t - m1)   or x without a corrector   (output 2: the next last_sample)
//   x_next = p_x x_c + p_m m_t + p_d (m1 - m_t)                                          (output 1)
// fp32 inside (explicit FMAs: thirteen roundings from the inputs to x_next), every output rounded to bf16 exactly once.
// HBM-bound row work: each byte is read once and written once; 16 bytes per lane where the nine plane starts share their offset from a
// 16-byte boundary, 2 bytes on the ragged ends and otherwise.  One H W plane of one (batch, frame, channel) per blockIdx.y step.
#include "ifx_common.h"

namespace ifx {
struct CfgUnipcArgs {
  const unsigned short *fc, *fu, *x, *last, *m1, *m2;
  unsigned short *x_next, *last_out, *m_out;
  long fc_sb, fc_sf, fc_sc, fu_sb, fu_sf, fu_sc;
  int frames, channels;
  long planes, plane;
  float guidance, sigma, c_last, c_m1, c_d1, c_dt, p_x, p_m, p_d;
  int corrector, c_order2, p_order2;
};

struct CfgUnipcOut {
  float x_next, x_c, m_t;
};

__device__ __forceinline__ CfgUnipcOut cfg_unipc_one(const CfgUnipcArgs& A, float fc, float fu, float x, float last, float m1, float m2) {
  const float flow = fmaf(A.guidance, fc - fu, fu);
  const float m_t = fmaf(-A.sigma, flow, x);
  float x_c = x;
  if (A.corrector) {
    x_c = A.c_last * last;
    x_c = fmaf(A.c_m1, m1, x_c);
    if (A.c_order2) x_c = fmaf(A.c_d1, m2 - m1, x_c);
    x_c = fmaf(A.c_dt, m_t - m1, x_c);
  }
  float x_next = A.p_x * x_c;
  x_next = fmaf(A.p_m, m_t, x_next);
  if (A.p_order2) x_next = fmaf(A.p_d, m1 - m_t, x_next);
  return {x_next, x_c, m_t};
}

__global__ __launch_bounds__(256) void cfg_unipc_step_kernel(CfgUnipcArgs A) {
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  for (long pl = blockIdx.y; pl < A.planes; pl += gridDim.y) {
    const long c = pl % A.channels, bf = pl / A.channels, f = bf % A.frames, b = bf / A.frames;
    const long off = pl * A.plane;
    // no __restrict__: the outputs may be the inputs (x_next on x, last_out on last, m_out on m2); an element is read in full, by
    // the one lane that owns it, before any of its three results is stored
    const unsigned short* fc = A.fc + b * A.fc_sb + f * A.fc_sf + c * A.fc_sc;
    const unsigned short* fu = A.fu + b * A.fu_sb + f * A.fu_sf + c * A.fu_sc;
    const unsigned short *x = A.x + off, *last = A.last + off, *m1 = A.m1 + off, *m2 = A.m2 + off;
    unsigned short *xn = A.x_next + off, *lo = A.last_out + off, *mo = A.m_out + off;
    // a slot that this step does not read (no corrector: last; order 1: m2; first step: m1) is handed over as x: same alignment, in bounds
    const unsigned mis = (unsigned)((uintptr_t)x & 15);
    const bool vec = ((uintptr_t)fc & 15) == mis && ((uintptr_t)fu & 15) == mis && ((uintptr_t)last & 15) == mis &&
                     ((uintptr_t)m1 & 15) == mis && ((uintptr_t)m2 & 15) == mis && ((uintptr_t)xn & 15) == mis &&
                     ((uintptr_t)lo & 15) == mis && ((uintptr_t)mo & 15) == mis;
    long head = vec ? (long)(((16u - mis) & 15u) >> 1) : A.plane;          // 2-byte elements in front of the 16-byte body
    if (head > A.plane) head = A.plane;
    const long nv = (A.plane - head) >> 3;                                  // 16-byte groups of the body
    const long tail0 = head + (nv << 3);                                    // scalar elements behind it: [tail0, plane)
    for (long i = tid; i < nv; i += stride) {
      const long e = head + (i << 3);
      const u16x8 vfc = *reinterpret_cast<const u16x8*>(fc + e), vfu = *reinterpret_cast<const u16x8*>(fu + e);
      const u16x8 vx = *reinterpret_cast<const u16x8*>(x + e), vl = *reinterpret_cast<const u16x8*>(last + e);
      const u16x8 v1 = *reinterpret_cast<const u16x8*>(m1 + e), v2 = *reinterpret_cast<const u16x8*>(m2 + e);
      u16x8 rn, rc, rm;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const CfgUnipcOut o = cfg_unipc_one(A, bf2f(vfc[k]), bf2f(vfu[k]), bf2f(vx[k]), bf2f(vl[k]), bf2f(v1[k]), bf2f(v2[k]));
        rn[k] = f2bf(o.x_next), rc[k] = f2bf(o.x_c), rm[k] = f2bf(o.m_t);
      }
      *reinterpret_cast<u16x8*>(xn + e) = rn;
      *reinterpret_cast<u16x8*>(lo + e) = rc;
      *reinterpret_cast<u16x8*>(mo + e) = rm;
    }
    const long n_scalar = head + (A.plane - tail0);
    for (long i = tid; i < n_scalar; i += stride) {
      const long e = i < head ? i : tail0 + (i - head);
      const CfgUnipcOut o = cfg_unipc_one(A, bf2f(fc[e]), bf2f(fu[e]), bf2f(x[e]), bf2f(last[e]), bf2f(m1[e]), bf2f(m2[e]));
      xn[e] = f2bf(o.x_next), lo[e] = f2bf(o.x_c), mo[e] = f2bf(o.m_t);
    }
  }
}
}  // namespace ifx

extern "C" int ifx_cfg_unipc_step(const ifx_cfg_unipc_step_desc* d, void* stream) {
  using namespace ifx;
  IFX_REQUIRE(d, "ifx_cfg_unipc_step: null descriptor");
  IFX_REQUIRE(d->flow_cond && d->flow_uncond && d->x && d->x_next && d->last_out && d->m_out,
              "ifx_cfg_unipc_step: null flow_cond, flow_uncond, x, x_next, last_out or m_out");
  IFX_REQUIRE(d->batch > 0 && d->frames > 0 && d->channels > 0 && d->plane > 0,
              "ifx_cfg_unipc_step: bad geometry (batch %d, frames %d, channels %d, H W %d)", d->batch, d->frames, d->channels, d->plane);
  IFX_REQUIRE((d->use_corrector == 0 || d->use_corrector == 1) && (d->corrector_order == 1 || d->corrector_order == 2) &&
                  (d->predictor_order == 1 || d->predictor_order == 2),
              "ifx_cfg_unipc_step: use_corrector %d (0 or 1), corrector order %d, predictor order %d (1 or 2)", d->use_corrector,
              d->corrector_order, d->predictor_order);
  const bool c2 = d->use_corrector && d->corrector_order == 2, p2 = d->predictor_order == 2;
  IFX_REQUIRE(!d->use_corrector || (d->last_sample && d->m1), "ifx_cfg_unipc_step: the corrector needs last_sample and m1");
  IFX_REQUIRE(!c2 || d->m2, "ifx_cfg_unipc_step: a corrector of order 2 needs m2");
  IFX_REQUIRE(!p2 || d->m1, "ifx_cfg_unipc_step: a predictor of order 2 needs m1");
  const void* ptrs[] = {d->flow_cond, d->flow_uncond, d->x, d->last_sample, d->m1, d->m2, d->x_next, d->last_out, d->m_out};
  for (const void* p : ptrs) IFX_REQUIRE(!((uintptr_t)p & 1), "ifx_cfg_unipc_step: a base pointer is not 2-byte aligned");
  const int64_t* strides[2] = {d->flow_cond_stride, d->flow_uncond_stride};
  const int32_t extent[3] = {d->batch, d->frames, d->channels};
  for (int s = 0; s < 2; ++s)
    for (int k = 0; k < 3; ++k)
      IFX_REQUIRE(extent[k] == 1 || strides[s][k] >= d->plane,
                  "ifx_cfg_unipc_step: %s stride %d is %ld elements, smaller than a plane of %d", s ? "flow_uncond" : "flow_cond", k,
                  (long)strides[s][k], d->plane);
  CfgUnipcArgs a{};
  a.fc = (const unsigned short*)d->flow_cond, a.fu = (const unsigned short*)d->flow_uncond, a.x = (const unsigned short*)d->x;
  a.last = d->use_corrector ? (const unsigned short*)d->last_sample : a.x;
  a.m1 = (d->use_corrector || p2) ? (const unsigned short*)d->m1 : a.x;
  a.m2 = c2 ? (const unsigned short*)d->m2 : a.x;
  a.x_next = (unsigned short*)d->x_next, a.last_out = (unsigned short*)d->last_out, a.m_out = (unsigned short*)d->m_out;
  a.fc_sb = d->flow_cond_stride[0], a.fc_sf = d->flow_cond_stride[1], a.fc_sc = d->flow_cond_stride[2];
  a.fu_sb = d->flow_uncond_stride[0], a.fu_sf = d->flow_uncond_stride[1], a.fu_sc = d->flow_uncond_stride[2];
  a.frames = d->frames, a.channels = d->channels;
  a.planes = (long)d->batch * d->frames * d->channels, a.plane = d->plane;
  a.guidance = d->guidance, a.sigma = d->sigma;
  a.c_last = d->c_last, a.c_m1 = d->c_m1, a.c_d1 = d->c_d1, a.c_dt = d->c_dt;
  a.p_x = d->p_x, a.p_m = d->p_m, a.p_d = d->p_d;
  a.corrector = d->use_corrector, a.c_order2 = c2, a.p_order2 = p2;
  // memory-bound: about eight workgroups per CU in all, the rest of a plane by grid stride
  const long gy = a.planes < 65535 ? a.planes : 65535;
  long gx = (a.plane / 8 + 255) / 256, cap = 2048 / gy;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(cfg_unipc_step_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("ifx_cfg_unipc_step");
}

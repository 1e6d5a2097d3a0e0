// ifx_attn_fwd_multi: the self-attention launches of several samples, each over its OWN cache, in one launch (concurrent sessions).
//
// The kernels are ifx_attn_pp.hip compiled a second time with PP_MULTI = 1: the same source text behind another prologue, so an
// item's tile sequence and per-tile arithmetic are those of its single launch by construction, and the kernels of ifx_attn_pp.hip
// (whose by-value AttnArgsPP must not grow) are not touched by this file's existence.
#define PP_MULTI 1
#include "ifx_attn_pp.hip"

namespace ifx {

// ifx_attn_fwd_multi: the instantiations of attn_fwd_multi_kernel are those of the schedules the automatic choice can pick (6 and 7),
// in both exponent forms and both matrix-instruction shapes, over contiguous and wave-uniform paged views.
int launch_attn_multi(const AttnMultiArgs& a, const AttnSchedule& s, int paged, AttnForm form, hipStream_t stream) {
  using namespace pp;
  const char* const what = "ifx_attn_fwd_multi";
  const AttnSchedule& own = attn_schedule(s.variant);
  int fr = form.pre ? own.fr_pre : own.fr;
  if (form.mfma16 && (fr == FR_U4 || fr == FR_U4_PRE)) fr = fr == FR_U4 ? FR_U4_M16 : FR_U4_PRE_M16;
  else if (form.mfma16) fr = -1;
  const dim3 grid(a.total), block(own.ng * 256);
#define PP_CASE(NG, FR)                                                                                                  \
  case (NG) * 16 + (FR):                                                                                                 \
    rc = paged ? launch_lds<attn_fwd_multi_kernel<1, false, NG, FR>>(grid, block, own.lds_bytes, stream, what, a)               \
               : launch_lds<attn_fwd_multi_kernel<0, false, NG, FR>>(grid, block, own.lds_bytes, stream, what, a);              \
    break
  int rc = IFX_OK;
  switch (fr < 0 || paged > 1 ? -1 : own.ng * 16 + fr) {
    PP_CASE(1, FR_U6_DUAL_PRE);
    PP_CASE(1, FR_U6_DUAL);
    PP_CASE(2, FR_U4_PRE);
    PP_CASE(2, FR_U4);
    PP_CASE(2, FR_U4_PRE_M16);
    PP_CASE(2, FR_U4_M16);
    default:
      set_error("ifx_attn_fwd_multi: no kernel built for variant %d in loop form %d (page kind %d)", s.variant, fr, paged);
      return IFX_EUNSUP;
  }
#undef PP_CASE
  if (rc != IFX_OK) return rc;
  return check_launch(what);
}

}  // namespace ifx

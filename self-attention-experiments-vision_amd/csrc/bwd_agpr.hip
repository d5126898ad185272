// bwd_agpr.hip -- attention kernels built for ONE wave per SIMD with the MFMA accumulators in the
// accumulator register file (AGPRs): this translation unit is compiled WITHOUT
// -amdgpu-mfma-vgpr-form (build.py), so a kernel can use the whole 512-register file (256 VGPRs
// for operands and softmax state + AGPRs for dK / dV) instead of the 256 VGPRs of the rest of the
// library.  Launchers only; the kernels live in the shared headers.
#include "bwd2_run.h"

namespace sae {

namespace {
#define SAE_ROW(name, pass, ...) \
  int name(hipStream_t st, const AttnArgs& a) { return bwd2_##pass##_run<__VA_ARGS__>(st, a); }
SAE_BWD2_AGPR_TABLE(SAE_ROW)
#undef SAE_ROW
}  // namespace

// head_dim 128 (BoTNet): the dQ pass at two waves per SIMD, the dK / dV pass at one
int bwd2_agpr128(hipStream_t st, const AttnArgs& a) {
  if (int rc = bwd2_dq_d128_agpr(st, a)) return rc;
  return bwd2_dkdv_d128_agpr(st, a);
}

// with relative logits at >= 128 keys: the dQ pass at one wave per SIMD (its relative-logit state
// spills at two).  The dK / dV pass that follows is attn.hip's bwd2_dkdv_d128_rel, the VGPR-form
// instance the 7 x 7 grid runs too: one definition, in one unit.
int bwd2_agpr128_rel_dq(hipStream_t st, const AttnArgs& a) { return bwd2_dq_d128_rel_agpr(st, a); }

}  // namespace sae

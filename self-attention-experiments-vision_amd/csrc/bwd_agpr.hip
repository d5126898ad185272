// bwd_agpr.hip -- attention kernels built for ONE wave per SIMD with the MFMA accumulators in the
// accumulator register file (AGPRs): this translation unit is compiled WITHOUT
// -amdgpu-mfma-vgpr-form (build.py), so a kernel can use the whole 512-register file (256 VGPRs
// for operands and softmax state + AGPRs for dK / dV) instead of the 256 VGPRs of the rest of the
// library.  Launchers only; the kernels live in the shared headers.
#include "bwd2_run.h"

namespace sae {

// head_dim 128 (BoTNet): the dQ pass at two waves per SIMD, the dK / dV pass at one
int bwd2_agpr128(hipStream_t st, const AttnArgs& a) { return bwd2_run<128, 4, 2, 4, 1>(st, a); }

// with relative logits at >= 128 keys: the dQ pass at one wave per SIMD (its relative-logit state
// spills at two).  The dK / dV pass that follows is attn.hip's attn_bwd2_dkdv_kernel<128, 4, 1,
// false, true>, the VGPR-form instance the 7 x 7 grid runs too: one definition, in one unit.
int bwd2_agpr128_rel_dq(hipStream_t st, const AttnArgs& a) { return bwd2_dq_run<128, 4, 1, false, true>(st, a); }

}  // namespace sae

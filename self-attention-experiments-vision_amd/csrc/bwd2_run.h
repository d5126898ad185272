// bwd2_run.h -- launchers of the lean bf16 two-pass backward (bwd2.h), shared by attn.hip and
// bwd_agpr.hip: a kernel instance belongs to the unit that names it here, and to that unit alone
// (tests/test_build_units_cpu.py).
#pragma once
#include "attn_kernels.h"
#include "bwd2.h"
#include "host.h"

namespace sae {

// dQ pass (publishes delta): NW waves x 32 query rows per workgroup, M waves per SIMD
template <int DP, int NW, int M, bool ROT = false, bool REL = false, bool DROP = false>
int bwd2_dq_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nq + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 4 * (size_t)F2<DP>::TILE + (REL ? 2 * kRelImg : 0);
  return launch("attn_bwd2_dq", attn_bwd2_dq_kernel<DP, NW, M, ROT, REL, DROP>, grid, dim3(64 * NW), lds, st, a);
}

// dK / dV pass: NW waves x 32 keys per workgroup
template <int DP, int NW, int M, bool ROT = false, bool REL = false, bool DROP = false>
int bwd2_dkdv_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nk + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 2 * (2 * (size_t)F2<DP>::TILE + 512 + (REL ? kRelImg : 0));
  return launch("attn_bwd2_dkdv", attn_bwd2_dkdv_kernel<DP, NW, M, ROT, REL, DROP>, grid, dim3(64 * NW), lds, st, a);
}

template <int DP, int NWQ, int MQ, int NWK, int MK, bool ROT = false, bool REL = false, bool DROP = false>
int bwd2_run(hipStream_t st, const AttnArgs& a) {
  if (int rc = bwd2_dq_run<DP, NWQ, MQ, ROT, REL, DROP>(st, a)) return rc;
  return bwd2_dkdv_run<DP, NWK, MK, ROT, REL, DROP>(st, a);
}

// bwd_agpr.hip: head_dim 128 with the accumulators in AGPRs -- both passes without relative
// logits; with them the dQ pass alone (its dK / dV pass is attn.hip's)
int bwd2_agpr128(hipStream_t st, const AttnArgs& a);
int bwd2_agpr128_rel_dq(hipStream_t st, const AttnArgs& a);

}  // namespace sae

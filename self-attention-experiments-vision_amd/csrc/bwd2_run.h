// bwd2_run.h -- instance tables and launchers of the lean bf16 two-pass backward (bwd2.h), shared
// by attn.hip and bwd_agpr.hip: a kernel instance is a row of ONE table here, and belongs to the
// unit that expands that table, and to that unit alone (tests/test_build_units_cpu.py).
#pragma once
#include "attn_kernels.h"
#include "bwd2.h"
#include "host.h"

namespace sae {

// dQ pass (publishes delta): NW waves x 32 query rows per workgroup, M waves per SIMD
template <int DP, int NW, int M, bool ROT, bool REL, bool DROP>
int bwd2_dq_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nq + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 4 * (size_t)F2<DP>::TILE + (REL ? 2 * kRelImg : 0);
  return launch("attn_bwd2_dq", attn_bwd2_dq_kernel<DP, NW, M, ROT, REL, DROP>, grid, dim3(64 * NW), lds, st, a);
}

// dK / dV pass: NW waves x 32 keys per workgroup
template <int DP, int NW, int M, bool ROT, bool REL, bool DROP>
int bwd2_dkdv_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nk + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 2 * (2 * (size_t)F2<DP>::TILE + 512 + (REL ? kRelImg : 0));
  return launch("attn_bwd2_dkdv", attn_bwd2_dkdv_kernel<DP, NW, M, ROT, REL, DROP>, grid, dim3(64 * NW), lds, st, a);
}

// attn.hip's instances.  Both passes run at two waves per SIMD except the dK / dV pass with
// relative logits at head_dim > 32 (one).
//  row name               DP   NW M  ROT    REL    DROP
#define SAE_BWD2_DQ_TABLE(X)                                  \
  X(bwd2_dq_d32,           32,  4, 2, false, false, false)    \
  X(bwd2_dq_d64,           64,  4, 2, false, false, false)    \
  X(bwd2_dq_d32_rot,       32,  4, 2, true,  false, false)    \
  X(bwd2_dq_d64_rot,       64,  4, 2, true,  false, false)    \
  X(bwd2_dq_d32_rel,       32,  4, 2, false, true,  false)    \
  X(bwd2_dq_d64_rel,       64,  4, 2, false, true,  false)    \
  X(bwd2_dq_d128_rel,      128, 4, 2, false, true,  false)    \
  X(bwd2_dq_d32_drop,      32,  4, 2, false, false, true)     \
  X(bwd2_dq_d64_drop,      64,  4, 2, false, false, true)
#define SAE_BWD2_DKDV_TABLE(X)                                \
  X(bwd2_dkdv_d32,         32,  4, 2, false, false, false)    \
  X(bwd2_dkdv_d64,         64,  4, 2, false, false, false)    \
  X(bwd2_dkdv_d32_rot,     32,  4, 2, true,  false, false)    \
  X(bwd2_dkdv_d64_rot,     64,  4, 2, true,  false, false)    \
  X(bwd2_dkdv_d32_rel,     32,  4, 2, false, true,  false)    \
  X(bwd2_dkdv_d64_rel,     64,  4, 1, false, true,  false)    \
  X(bwd2_dkdv_d128_rel,    128, 4, 1, false, true,  false)    \
  X(bwd2_dkdv_d32_drop,    32,  4, 2, false, false, true)     \
  X(bwd2_dkdv_d64_drop,    64,  4, 2, false, false, true)

// bwd_agpr.hip's instances: head_dim 128 with the accumulators in AGPRs.  attn.hip launches them
// through that unit's two functions and never expands this table.
//  row name               pass  DP   NW M  ROT    REL    DROP
#define SAE_BWD2_AGPR_TABLE(X)                                     \
  X(bwd2_dq_d128_agpr,     dq,   128, 4, 2, false, false, false)   \
  X(bwd2_dkdv_d128_agpr,   dkdv, 128, 4, 1, false, false, false)   \
  X(bwd2_dq_d128_rel_agpr, dq,   128, 4, 1, false, true,  false)

// bwd2_dq_d128_agpr then bwd2_dkdv_d128_agpr
int bwd2_agpr128(hipStream_t st, const AttnArgs& a);
// bwd2_dq_d128_rel_agpr alone (its dK / dV pass is attn.hip's bwd2_dkdv_d128_rel)
int bwd2_agpr128_rel_dq(hipStream_t st, const AttnArgs& a);

}  // namespace sae

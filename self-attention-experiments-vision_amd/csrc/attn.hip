// attn.hip -- the attention entry points of the C ABI (include/sae_attn.h): template dispatch and
// stream-ordered launches of the fused attention core, the relative-logit tables and rotary.
#include <type_traits>

#include "attn_kernels.h"
#include "variants.h"
#include "fwd2.h"
#include "bwd2_run.h"
#include "bwd3.h"
#include "cls.h"
#include "desc.h"

namespace sae {

// ------------------------------------------------------------------------ dropout: standalone kernels
// keep[b][h][q][k] as uint8 0 / 1: one thread per element (a test and debugging aid)
struct DropMaskArgs {
  const unsigned long long* rng;
  unsigned char* keep;
  long long n;
  int H, Nq, Nk;
  unsigned stream_id, thr;
};

__global__ void dropout_mask_kernel(DropMaskArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const DropKey dk = drop_key(a.rng, a.stream_id);
  const unsigned k = (unsigned)(i % a.Nk);
  const long long t = i / a.Nk;
  const unsigned q = (unsigned)(t % a.Nq);
  const unsigned bh = (unsigned)(t / a.Nq);
  a.keep[i] = drop_keep(dk, a.thr, bh, q, k) ? 1 : 0;
}

// offset += n on the stream (the next step's masks)
__global__ void dropout_advance_kernel(unsigned long long* rng, unsigned long long n) {
  if (threadIdx.x == 0) rng[1] += n;
}

}  // namespace sae

using namespace sae;

namespace {

void fill_args(AttnArgs& a, const sae_attn_desc* d) {
  fill_desc(a, d);
  if (d->flags & SAE_FLAG_RELPOS) {
    a.rel_h = d->rel_h;
    a.rel_w = d->rel_w;
    a.rel_magic = div_magic(d->rel_w);
  }
}

// ------------------------------------------------------------------------- v1 launchers
// The v1 kernels (attn_kernels.h) cover the whole envelope: fp32, unaligned strides or head_dim,
// relative logits on grids up to 64 x 64, dropout (REL && DROP is never instantiated).
struct V1 {
  int dtype, dp;
  bool vec, rel, drop;
};

int rel_lds_floats(const AttnArgs& a) { return a.rel_h ? 32 * (a.rel_h + a.rel_w + 1) : 0; }

template <typename T, int DP, bool VEC, bool REL, bool DROP> struct FwdL {
  static int run(hipStream_t st, const AttnArgs& a) {
    const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK) + (REL ? 4 * rel_lds_floats(a) * sizeof(float) : 0);
    return launch(DROP ? "attn_fwd_drop" : "attn_fwd", attn_fwd_kernel<T, DP, VEC, REL, DROP>, grid, dim3(256), lds, st,
                  a);
  }
};

template <typename T, int DP, bool VEC, bool REL, bool DROP> struct BwdL {
  static int run(hipStream_t st, const AttnArgs& a) {
    {  // dQ (+ delta) first: it publishes delta for the dK/dV pass
      const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
      const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK) + (REL ? 8 * rel_lds_floats(a) * sizeof(float) : 0);
      if (int rc = launch(DROP ? "attn_bwd_dq_drop" : "attn_bwd_dq", attn_bwd_dq_kernel<T, DP, VEC, REL, DROP>, grid,
                          dim3(256), lds, st, a))
        return rc;
    }
    const long long grid = (long long)((a.Nk + kBKV - 1) / kBKV) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * (2 * Img<T, DP>::bytes(kBQT) + 2 * kBQT * sizeof(float) +
                                        (REL ? (size_t)kBQT * (a.rel_h + a.rel_w + 1) * sizeof(float) : 0));
    return launch(DROP ? "attn_bwd_dkdv_drop" : "attn_bwd_dkdv", attn_bwd_dkdv_kernel<T, DP, VEC, REL, DROP>, grid,
                  dim3(256), lds, st, a);
  }
};

template <template <typename, int, bool, bool, bool> class L, typename T, int DP, bool VEC>
int v1_run(const V1& v, hipStream_t st, const AttnArgs& a) {
  if (v.drop) return L<T, DP, VEC, false, true>::run(st, a);
  return v.rel ? L<T, DP, VEC, true, false>::run(st, a) : L<T, DP, VEC, false, false>::run(st, a);
}

template <template <typename, int, bool, bool, bool> class L>
int dispatch(const V1& v, hipStream_t st, const AttnArgs& a) {
#define SAE_CASE(T, DPV) \
  if (v.dp == DPV) return v.vec ? v1_run<L, T, DPV, true>(v, st, a) : v1_run<L, T, DPV, false>(v, st, a);
  if (v.dtype == SAE_DTYPE_BF16) {
    SAE_CASE(__bf16, 32) SAE_CASE(__bf16, 64) SAE_CASE(__bf16, 128)
  } else {
    SAE_CASE(float, 32) SAE_CASE(float, 64) SAE_CASE(float, 128)
  }
#undef SAE_CASE
  return fail(SAE_EUNSUPPORTED, "no kernel instance for dtype %d dp %d", v.dtype, v.dp);
}

// ------------------------------------------------------------------- lean kernel launchers
// lean bf16 forward (fwd2.h): NW waves x 32 query rows per workgroup
template <int DP, int NW, int MINW, bool LSUM, bool ROT, int NSU, bool REL, bool FIX, bool DROP>
int fwd2_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nq + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 4 * (size_t)F2<DP>::TILE + (REL ? 2 * kRelImg : 0);
  return launch("attn_fwd2", attn_fwd2_kernel<DP, NW, MINW, LSUM, ROT, NSU, REL, FIX, DROP>, grid, dim3(64 * NW), lds, st, a);
}

// single-pass bf16 backward (bwd3.h): one workgroup per (batch, head) holding all Nk <= 256 keys
// (8 waves x 32 keys, two waves per SIMD); longer key ranges take the two-pass bwd2
constexpr int kB3Keys = 256;

template <int DP, int NW, int KPW, bool ROT, int NSU, bool DROP>
int bwd3_run(hipStream_t st, const AttnArgs& a) {
  using C = B3<DP, NW, KPW>;
  static_assert(C::BK == kB3Keys, "bwd3 dispatch assumes 256-key blocks");
  if (a.Nk > C::BK) return fail(SAE_EINVAL, "bwd3: %d keys > %d", a.Nk, C::BK);
  return launch("attn_bwd3", attn_bwd3_kernel<DP, NW, KPW, ROT, NSU, DROP>, (long long)a.H * a.B, dim3(64 * NW), C::LDS, st,
                a);
}

// single query row (CaiT class attention, CeiT LCA): the K/V stream kernels of cls.h, NCH 64-wide
// head_dim chunks per row
constexpr int kClsMaxKeys = 1 << 20;
template <bool BWD, int NCH> int cls_run(hipStream_t st, const AttnArgs& a) {
  return launch(BWD ? "attn_cls_bwd" : "attn_cls_fwd", BWD ? attn_cls_bwd_kernel<NCH> : attn_cls_fwd_kernel<NCH>,
                (long long)a.B * a.H, dim3(256), cls_lds_bytes<NCH>(), st, a);
}

// ------------------------------------------------------------------------ instance tables
// Every instance of the lean bf16 kernels this unit holds is ONE row here (the two-pass backward's
// rows are in bwd2_run.h): the template parameters are written once, under their names, and every
// launch refers to the row's name.  A new instance is a new row, never a tuple at a call site.
//
// The lean forward's variant per padded head dim:
//   DP <= 64: three waves per SIMD, row sum on the VALU, running max fixed by the first tile (FIX,
//             with the tracking sweep as the in-kernel fallback): 23.2 vs 24.6 us at DeiT-S, 95.4 vs
//             96.5 us at ViT-B@384 (profiles/r03b_fwdvar.txt, bitwise-equal outputs).  head_dim <= 48
//             (CaiT) in 64-wide tiles without rotary: QK^T skips the all-zero fourth k-step (NSU 3).
//             The rotary instances take the same variant: the fused-rotary forward stays bit-equal
//             to the standalone rotary pass + this forward (tests/test_gpu_rotary.py).
//   DP 128:   two waves per SIMD, row sum on the MFMA (the VALU row sum is 2x slower there,
//             profiles/r01_attn_fwd_f0_vs_f6_interleaved_v13.txt).
//   REL:      BoTNet relative logits, two waves per SIMD, row sum on the MFMA.
//   DROP:     the DP <= 64 variant with the dropped P zeroed; at DP 64 the Philox state does not fit
//             three waves per SIMD (5 / 16 VGPRs spilled): two there.
//  row name         DP   NW MINW LSUM   ROT    NSU REL    FIX    DROP
#define SAE_FWD2_TABLE(X)                                              \
  X(fwd2_d32,        32,  4, 3,   false, false, 2,  false, true,  false) \
  X(fwd2_d64_k3,     64,  4, 3,   false, false, 3,  false, true,  false) \
  X(fwd2_d64,        64,  4, 3,   false, false, 4,  false, true,  false) \
  X(fwd2_d128,       128, 4, 2,   true,  false, 8,  false, false, false) \
  X(fwd2_d32_rot,    32,  4, 3,   false, true,  2,  false, true,  false) \
  X(fwd2_d64_rot,    64,  4, 3,   false, true,  4,  false, true,  false) \
  X(fwd2_d32_rel,    32,  4, 2,   true,  false, 2,  true,  false, false) \
  X(fwd2_d64_rel,    64,  4, 2,   true,  false, 4,  true,  false, false) \
  X(fwd2_d128_rel,   128, 4, 2,   true,  false, 8,  true,  false, false) \
  X(fwd2_d32_drop,   32,  4, 3,   false, false, 2,  false, true,  true)  \
  X(fwd2_d64_k3_drop, 64, 4, 2,   false, false, 3,  false, true,  true)  \
  X(fwd2_d64_drop,   64,  4, 2,   false, false, 4,  false, true,  true)

// (waves 4-7 staggered, the previous tile's dQ first: DeiT-S 53.6 -> 53.2 us, CaiT-S24
// 130.7 -> 128.3 us, profiles/r06g_bwd3_stagger_ab.txt; same sums, bit-identical results)
//  row name         DP  NW KPW ROT    NSU DROP
#define SAE_BWD3_TABLE(X)                            \
  X(bwd3_d32,        32, 8, 1,  false, 2,  false)    \
  X(bwd3_d64_k3,     64, 8, 1,  false, 3,  false)    \
  X(bwd3_d64,        64, 8, 1,  false, 4,  false)    \
  X(bwd3_d32_rot,    32, 8, 1,  true,  2,  false)    \
  X(bwd3_d64_rot,    64, 8, 1,  true,  4,  false)    \
  X(bwd3_d32_drop,   32, 8, 1,  false, 2,  true)     \
  X(bwd3_d64_k3_drop, 64, 8, 1, false, 3,  true)     \
  X(bwd3_d64_drop,   64, 8, 1,  false, 4,  true)

//  row name         BWD    NCH
#define SAE_CLS_TABLE(X)          \
  X(cls_fwd_1,       false, 1)    \
  X(cls_fwd_2,       false, 2)    \
  X(cls_bwd_1,       true,  1)    \
  X(cls_bwd_2,       true,  2)

// one launch of a route: a table row, one of bwd_agpr.hip's two functions, or the v1 launcher
#define SAE_ROW(name, ...) name,
enum class Inst {
  SAE_FWD2_TABLE(SAE_ROW) SAE_BWD3_TABLE(SAE_ROW) SAE_BWD2_DQ_TABLE(SAE_ROW) SAE_BWD2_DKDV_TABLE(SAE_ROW)
  SAE_CLS_TABLE(SAE_ROW)
  bwd2_d128_agpr,          // bwd2_agpr128: both passes
  bwd2_dq_d128_rel_agpr,   // bwd2_agpr128_rel_dq
  v1_fwd,
  v1_bwd,
};
#undef SAE_ROW

const char* inst_name(Inst i) {
  switch (i) {
#define SAE_ROW(name, ...) \
  case Inst::name: return #name;
    SAE_FWD2_TABLE(SAE_ROW) SAE_BWD3_TABLE(SAE_ROW) SAE_BWD2_DQ_TABLE(SAE_ROW) SAE_BWD2_DKDV_TABLE(SAE_ROW)
    SAE_CLS_TABLE(SAE_ROW)
#undef SAE_ROW
    case Inst::bwd2_d128_agpr: return "bwd2_dq_d128_agpr+bwd2_dkdv_d128_agpr";   // SAE_BWD2_AGPR_TABLE's names
    case Inst::bwd2_dq_d128_rel_agpr: return "bwd2_dq_d128_rel_agpr";
    case Inst::v1_fwd: return "v1_fwd";
    case Inst::v1_bwd: return "v1_bwd";
  }
  return "?";
}

int run_inst(Inst i, const V1& v1, hipStream_t st, const AttnArgs& a) {
  switch (i) {
#define SAE_F2(name, ...) \
  case Inst::name: return fwd2_run<__VA_ARGS__>(st, a);
#define SAE_B3(name, ...) \
  case Inst::name: return bwd3_run<__VA_ARGS__>(st, a);
#define SAE_DQ(name, ...) \
  case Inst::name: return bwd2_dq_run<__VA_ARGS__>(st, a);
#define SAE_DKDV(name, ...) \
  case Inst::name: return bwd2_dkdv_run<__VA_ARGS__>(st, a);
#define SAE_CLS(name, ...) \
  case Inst::name: return cls_run<__VA_ARGS__>(st, a);
    SAE_FWD2_TABLE(SAE_F2) SAE_BWD3_TABLE(SAE_B3) SAE_BWD2_DQ_TABLE(SAE_DQ) SAE_BWD2_DKDV_TABLE(SAE_DKDV)
    SAE_CLS_TABLE(SAE_CLS)
#undef SAE_F2
#undef SAE_B3
#undef SAE_DQ
#undef SAE_DKDV
#undef SAE_CLS
    case Inst::bwd2_d128_agpr: return bwd2_agpr128(st, a);
    case Inst::bwd2_dq_d128_rel_agpr: return bwd2_agpr128_rel_dq(st, a);
    case Inst::v1_fwd: return dispatch<FwdL>(v1, st, a);
    case Inst::v1_bwd: return dispatch<BwdL>(v1, st, a);
  }
  return fail(SAE_EINVAL, "attention: bad instance %d", (int)i);
}

// ------------------------------------------------------------------------------- the plan
// The one routing decision of the attention entry points: sae_attn_route reports it, the entry
// points launch it.  Pure: no HIP call, no pointer; the caller reads the dev knob.
struct AttnFacts {
  int pass, form;   // SAE_PASS_*, SAE_FORM_*
  int dtype, D, dp, Nq, Nk;
  bool vec;         // desc_vec: 16-byte aligned strides, head_dim and pointers
  int rel_cols;     // rel_h + rel_w with SAE_FLAG_RELPOS, else 0
  int var;          // SAE_FWD_VARIANT / SAE_BWD_VARIANT: 1 forces v1, 2 (backward) skips bwd3
};

struct AttnPlan {
  int n;
  Inst step[2];
  V1 v1;   // the v1 steps' instance
};

int route(AttnPlan* p, Inst s0) {
  p->n = 1;
  p->step[0] = s0;
  return SAE_OK;
}
int route(AttnPlan* p, Inst s0, Inst s1) {
  p->n = 2;
  p->step[0] = s0;
  p->step[1] = s1;
  return SAE_OK;
}

int attn_plan(const AttnFacts& f, AttnPlan* p) {
  using I = Inst;
  const bool bwd = f.pass == SAE_PASS_BWD, bf16 = f.dtype == SAE_DTYPE_BF16, rel = f.rel_cols > 0;
  const bool d32 = f.dp == 32;
  const bool k3 = f.dp == 64 && f.D <= 48;    // CaiT head_dim 48 in 64-wide tiles: three k-steps
  const bool one_pass = f.Nk <= kB3Keys;      // bwd3 holds every key in one workgroup
  p->v1 = V1{f.dtype, f.dp, f.vec, rel, f.form == SAE_FORM_DROPOUT};

  if (f.form == SAE_FORM_ROTARY) {   // rotary rides on the lean bf16 kernels only
    if (!bf16 || !f.vec || rel || f.dp > 64)
      return fail(SAE_EUNSUPPORTED, "rotary: fused only on the bf16 path with head_dim <= 64 (16-byte aligned "
                  "strides, no flags)");
    if (!bwd) return route(p, d32 ? I::fwd2_d32_rot : I::fwd2_d64_rot);
    if (one_pass) return route(p, d32 ? I::bwd3_d32_rot : I::bwd3_d64_rot);
    return d32 ? route(p, I::bwd2_dq_d32_rot, I::bwd2_dkdv_d32_rot) : route(p, I::bwd2_dq_d64_rot, I::bwd2_dkdv_d64_rot);
  }

  if (f.form == SAE_FORM_DROPOUT) {
    // the lean kernels' DROP instances: aligned strides, head_dim <= 64, more than one query row;
    // the v1 DROP instances cover the rest of the plain envelope
    if (bf16 && f.vec && f.dp <= 64 && f.Nq > 1) {
      if (!bwd) return route(p, d32 ? I::fwd2_d32_drop : k3 ? I::fwd2_d64_k3_drop : I::fwd2_d64_drop);
      if (one_pass) return route(p, d32 ? I::bwd3_d32_drop : k3 ? I::bwd3_d64_k3_drop : I::bwd3_d64_drop);
      return d32 ? route(p, I::bwd2_dq_d32_drop, I::bwd2_dkdv_d32_drop)
                 : route(p, I::bwd2_dq_d64_drop, I::bwd2_dkdv_d64_drop);
    }
    return route(p, bwd ? I::v1_bwd : I::v1_fwd);
  }

  const bool lean = f.var != 1 && bf16 && f.vec;
  if (lean && !rel && f.Nq == 1 && f.Nk <= kClsMaxKeys) {
    if (bwd) return route(p, f.D > 64 ? I::cls_bwd_2 : I::cls_bwd_1);
    return route(p, f.D > 64 ? I::cls_fwd_2 : I::cls_fwd_1);
  }
  if (lean && !rel) {
    if (!bwd) return route(p, d32 ? I::fwd2_d32 : k3 ? I::fwd2_d64_k3 : f.dp == 64 ? I::fwd2_d64 : I::fwd2_d128);
    if (one_pass && f.var != 2 && f.dp <= 64) return route(p, d32 ? I::bwd3_d32 : k3 ? I::bwd3_d64_k3 : I::bwd3_d64);
    if (d32) return route(p, I::bwd2_dq_d32, I::bwd2_dkdv_d32);
    if (f.dp == 64) return route(p, I::bwd2_dq_d64, I::bwd2_dkdv_d64);
    // head_dim 128 (BoTNet): the dK / dV pass at one wave per SIMD (the dK / dV accumulators of 32
    // keys x 128 columns plus the K / V fragments need more than half the register file), built in
    // the AGPR translation unit (bwd_agpr.hip: accumulators in AGPRs, no spills; bot14 bwd
    // 222 -> 216 us, bot7 49 -> 47 us same box, profiles/r03f_bot_agpr_ab.txt)
    return route(p, I::bwd2_d128_agpr);
  }
  // BoTNet relative logits on the lean kernels: the table columns (Hs + Ws) fit the two extra
  // score k-steps; larger grids (up to 64 x 64) and fp32 take the v1 kernels
  if (lean && rel && f.rel_cols <= kRelCols) {
    if (!bwd) return route(p, d32 ? I::fwd2_d32_rel : f.dp == 64 ? I::fwd2_d64_rel : I::fwd2_d128_rel);
    if (d32) return route(p, I::bwd2_dq_d32_rel, I::bwd2_dkdv_d32_rel);
    if (f.dp == 64) return route(p, I::bwd2_dq_d64_rel, I::bwd2_dkdv_d64_rel);
    // head_dim 128 with relative logits: at 14 x 14 the dQ pass at one wave per SIMD in the AGPR
    // unit (its relative-logit state spills 75 VGPRs at two waves per SIMD): bot14+rel bwd
    // 315 -> 298 us; the 7 x 7 grid keeps the two-wave dQ pass (59 vs 67 us).  The dK / dV pass
    // is this unit's instance at either size.
    return route(p, f.Nk < 128 ? I::bwd2_dq_d128_rel : I::bwd2_dq_d128_rel_agpr, I::bwd2_dkdv_d128_rel);
  }
  return route(p, bwd ? I::v1_bwd : I::v1_fwd);
}

AttnFacts attn_facts(const sae_attn_desc* d, int pass, int form, bool vec) {
  return AttnFacts{pass, form, d->dtype, d->head_dim, pick_dp(d->head_dim), d->seq_q, d->seq_k, vec,
                   (d->flags & SAE_FLAG_RELPOS) ? d->rel_h + d->rel_w : 0,
                   dev_knob(pass == SAE_PASS_BWD ? "SAE_BWD_VARIANT" : "SAE_FWD_VARIANT")};
}

int run_plan(const AttnPlan& p, hipStream_t st, const AttnArgs& a) {
  for (int i = 0; i < p.n; ++i)
    if (int rc = run_inst(p.step[i], p.v1, st, a)) return rc;
  return SAE_OK;
}

// the route's name: its launches in order, the v1 steps with their instance
std::string plan_name(const AttnPlan& p) {
  std::string s;
  for (int i = 0; i < p.n; ++i) {
    s += i ? "+" : "";
    if (p.step[i] != Inst::v1_fwd && p.step[i] != Inst::v1_bwd) {
      s += inst_name(p.step[i]);
      continue;
    }
    const std::string inst = std::string(p.v1.dtype == SAE_DTYPE_BF16 ? "_bf16_d" : "_f32_d") + std::to_string(p.v1.dp) +
                             (p.v1.vec ? "" : "_scalar") + (p.v1.rel ? "_rel" : p.v1.drop ? "_drop" : "");
    s += p.step[i] == Inst::v1_fwd ? "v1_fwd" + inst : "v1_bwd_dq" + inst + "+v1_bwd_dkdv" + inst;   // BwdL: two passes
  }
  return s;
}

// ------------------------------------------------------------------------------- dropout
// Attention-probability dropout (dropout.h) on the envelope of the plain entry points with
// flags == 0.
struct DropCall {
  const unsigned long long* rng;
  unsigned stream_id, thr;
};

void fill_drop(AttnArgs& a, const DropCall& c) {
  a.drop_rng = c.rng;
  a.drop_stream = c.stream_id;
  a.drop_thr = c.thr;
  a.drop_inv = 256.f / (float)(256 - (int)c.thr);
}

int drop_desc_check(const sae_attn_desc* d) {
  if (!d) return fail(SAE_EINVAL, "desc is NULL");
  if (d->flags != 0)
    return fail(SAE_EUNSUPPORTED, "dropout: flags 0x%x are not supported (no relative logits)", d->flags);
  return SAE_OK;
}

// T = clamp(lrintf(rate * 256), 0, 255): a rate below 1 / 512 rounds to T = 0, no dropout
int drop_check(const sae_attn_desc* d, float rate, const uint64_t* rng, unsigned* thr) {
  if (!(rate >= 0.f && rate < 1.f)) return fail(SAE_EINVAL, "dropout rate %g is outside [0, 1)", (double)rate);
  if (!rng) return fail(SAE_EINVAL, "dropout: rng must be non-NULL");
  if (int rc = drop_desc_check(d)) return rc;
  *thr = (unsigned)std::min(255L, std::max(0L, lrintf(rate * 256.f)));
  return SAE_OK;
}

// ------------------------------------------------------- entry points: validate, fill, plan, launch
int attn_fwd_impl(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                  const float* bias_h, const float* bias_w, void* o, float* lse, const RopeTab* rope,
                  const DropCall* drop = nullptr) {
  int rc = validate(d, false);
  if (rc) return rc;
  if (!q || !k || !v || !o) return fail(SAE_EINVAL, "q/k/v/o must be non-NULL");
  if ((d->flags & SAE_FLAG_RELPOS) && (!bias_h || !bias_w))
    return fail(SAE_EINVAL, "SAE_FLAG_RELPOS needs bias_h and bias_w");
  AttnArgs a;
  fill_args(a, d);
  a.q = q;
  a.k = k;
  a.v = v;
  a.out = o;
  a.lse = lse;
  a.bias_h = bias_h;
  a.bias_w = bias_w;
  if (rope) a.rope = *rope;
  if (drop) fill_drop(a, *drop);
  AttnPlan p;
  const int form = rope ? SAE_FORM_ROTARY : drop ? SAE_FORM_DROPOUT : SAE_FORM_PLAIN;
  if ((rc = attn_plan(attn_facts(d, SAE_PASS_FWD, form, desc_vec(d, {q, k, v, o}, false)), &p))) return rc;
  return run_plan(p, (hipStream_t)stream, a);
}

int attn_bwd_impl(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                  const void* o, const float* lse, const void* dout, const float* bias_h,
                  const float* bias_w, void* dq, void* dk, void* dv, float* dbias_h, float* dbias_w,
                  void* workspace, const RopeTab* rope, const DropCall* drop = nullptr) {
  int rc = validate(d, true);
  if (rc) return rc;
  if (!q || !k || !v || !o || !lse || !dout || !dq || !dk || !dv || !workspace)
    return fail(SAE_EINVAL, "q/k/v/o/lse/dout/dq/dk/dv/workspace must be non-NULL");
  if ((d->flags & SAE_FLAG_RELPOS) && (!bias_h || !bias_w || !dbias_h || !dbias_w))
    return fail(SAE_EINVAL, "SAE_FLAG_RELPOS needs bias_h, bias_w, dbias_h, dbias_w");
  AttnArgs a;
  fill_args(a, d);
  a.q = q;
  a.k = k;
  a.v = v;
  a.o = o;
  a.lse = const_cast<float*>(lse);
  a.dout = dout;
  a.dq = dq;
  a.dk = dk;
  a.dv = dv;
  a.delta = reinterpret_cast<float*>(workspace);
  a.bias_h = bias_h;
  a.bias_w = bias_w;
  a.dbias_h = dbias_h;
  a.dbias_w = dbias_w;
  if (rope) a.rope = *rope;
  if (drop) fill_drop(a, *drop);
  AttnPlan p;
  const int form = rope ? SAE_FORM_ROTARY : drop ? SAE_FORM_DROPOUT : SAE_FORM_PLAIN;
  if ((rc = attn_plan(attn_facts(d, SAE_PASS_BWD, form, desc_vec(d, {q, k, v, o, dout, dq, dk, dv}, true)), &p)))
    return rc;
  return run_plan(p, (hipStream_t)stream, a);
}

int rel_validate(int B, int H, int Hs, int Ws, int D, int dtype) {
  if (B < 1 || H < 1 || Hs < 1 || Ws < 1 || D < 1) return fail(SAE_EINVAL, "relpos sizes must be >= 1");
  if (dtype != SAE_DTYPE_BF16 && dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "bad dtype %d", dtype);
  if (Hs > 64 || Ws > 64) return fail(SAE_EUNSUPPORTED, "relpos grid %dx%d exceeds 64x64", Hs, Ws);
  return SAE_OK;
}

// elementwise kernels: one thread per element, 256 per workgroup
long long blocks256(long long n) { return (n + 255) / 256; }

}  // namespace

extern "C" {

void sae_attn_desc_init(sae_attn_desc* d, int32_t batch, int32_t heads, int32_t seq_q, int32_t seq_k,
                        int32_t head_dim, int32_t dtype, float scale) {
  memset(d, 0, sizeof *d);
  d->batch = batch;
  d->heads = heads;
  d->seq_q = seq_q;
  d->seq_k = seq_k;
  d->head_dim = head_dim;
  d->dtype = dtype;
  d->scale = scale;
  const int64_t hq[3] = {(int64_t)seq_q * heads * head_dim, (int64_t)heads * head_dim, head_dim};
  const int64_t hk[3] = {(int64_t)seq_k * heads * head_dim, (int64_t)heads * head_dim, head_dim};
  for (int i = 0; i < 3; ++i) {
    d->q_stride[i] = d->o_stride[i] = d->do_stride[i] = d->dq_stride[i] = hq[i];
    d->k_stride[i] = d->v_stride[i] = d->dk_stride[i] = d->dv_stride[i] = hk[i];
  }
}

int sae_attn_fwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                 const float* bias_h, const float* bias_w, void* o, float* lse) {
  return attn_fwd_impl(stream, d, q, k, v, bias_h, bias_w, o, lse, nullptr);
}

int sae_attn_fwd_rotary(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                        const float* sin_tab, const float* cos_tab, void* o, float* lse) {
  if (!d) return fail(SAE_EINVAL, "NULL descriptor");
  if (int rc = rope_check(d, sin_tab, cos_tab)) return rc;
  const RopeTab t = make_rope(d, sin_tab, cos_tab);
  return attn_fwd_impl(stream, d, q, k, v, nullptr, nullptr, o, lse, &t);
}

size_t sae_attn_bwd_workspace_bytes(const sae_attn_desc* d) { return d ? delta_bytes(d) : 0; }

int sae_attn_bwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                 const void* o, const float* lse, const void* dout, const float* bias_h, const float* bias_w,
                 void* dq, void* dk, void* dv, float* dbias_h, float* dbias_w, void* workspace) {
  return attn_bwd_impl(stream, d, q, k, v, o, lse, dout, bias_h, bias_w, dq, dk, dv, dbias_h, dbias_w, workspace,
                       nullptr);
}

int sae_attn_bwd_rotary(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                        const void* o, const float* lse, const void* dout, const float* sin_tab,
                        const float* cos_tab, void* dq, void* dk, void* dv, void* workspace) {
  if (!d) return fail(SAE_EINVAL, "NULL descriptor");
  if (int rc = rope_check(d, sin_tab, cos_tab)) return rc;
  const RopeTab t = make_rope(d, sin_tab, cos_tab);
  return attn_bwd_impl(stream, d, q, k, v, o, lse, dout, nullptr, nullptr, dq, dk, dv, nullptr, nullptr, workspace,
                       &t);
}

// host-only: the plan of the entry point of that pass and form, by name (no HIP call)
const char* sae_attn_route(const sae_attn_desc* d, int32_t pass, int32_t form, int32_t aligned) {
  static thread_local std::string name;
  if (route_args_check(pass, form)) return nullptr;
  if (form == SAE_FORM_ROTARY) {
    if (!d) return fail(SAE_EINVAL, "NULL descriptor"), nullptr;
    if (rope_dim_check(d)) return nullptr;
  }
  if (form == SAE_FORM_DROPOUT && drop_desc_check(d)) return nullptr;
  const bool bwd = pass == SAE_PASS_BWD;
  if (validate(d, bwd)) return nullptr;
  AttnPlan p;
  if (attn_plan(attn_facts(d, pass, form, aligned && desc_strides_vec(d, bwd)), &p)) return nullptr;
  name = plan_name(p);
  ok();
  return name.c_str();
}

// --------------------------------------------------------------------------------- dropout
int sae_attn_fwd_dropout(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v, void* o,
                         float* lse, float rate, const uint64_t* rng, uint32_t stream_id) {
  unsigned thr = 0;
  if (int rc = drop_check(d, rate, rng, &thr)) return rc;
  if (thr == 0) return attn_fwd_impl(stream, d, q, k, v, nullptr, nullptr, o, lse, nullptr);
  const DropCall c{reinterpret_cast<const unsigned long long*>(rng), stream_id, thr};
  return attn_fwd_impl(stream, d, q, k, v, nullptr, nullptr, o, lse, nullptr, &c);
}

int sae_attn_bwd_dropout(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                         const void* o, const float* lse, const void* dout, void* dq, void* dk, void* dv,
                         void* workspace, float rate, const uint64_t* rng, uint32_t stream_id) {
  unsigned thr = 0;
  if (int rc = drop_check(d, rate, rng, &thr)) return rc;
  if (thr == 0)
    return attn_bwd_impl(stream, d, q, k, v, o, lse, dout, nullptr, nullptr, dq, dk, dv, nullptr, nullptr, workspace,
                         nullptr);
  const DropCall c{reinterpret_cast<const unsigned long long*>(rng), stream_id, thr};
  return attn_bwd_impl(stream, d, q, k, v, o, lse, dout, nullptr, nullptr, dq, dk, dv, nullptr, nullptr, workspace,
                       nullptr, &c);
}

int sae_attn_dropout_mask(void* stream, int32_t B, int32_t H, int32_t Nq, int32_t Nk, float rate, const uint64_t* rng,
                          uint32_t stream_id, uint8_t* keep) {
  if (!(rate >= 0.f && rate < 1.f)) return fail(SAE_EINVAL, "dropout rate %g is outside [0, 1)", (double)rate);
  if (!rng || !keep) return fail(SAE_EINVAL, "dropout: rng and keep must be non-NULL");
  if (B < 1 || H < 1 || Nq < 1 || Nk < 1) return fail(SAE_EINVAL, "dropout mask sizes must be >= 1");
  DropMaskArgs a;
  memset(&a, 0, sizeof a);
  a.rng = reinterpret_cast<const unsigned long long*>(rng);
  a.keep = keep;
  a.n = (long long)B * H * Nq * Nk;
  a.H = H;
  a.Nq = Nq;
  a.Nk = Nk;
  a.stream_id = stream_id;
  a.thr = (unsigned)std::min(255L, std::max(0L, lrintf(rate * 256.f)));
  return launch("dropout_mask", dropout_mask_kernel, blocks256(a.n), dim3(256), 0, (hipStream_t)stream, a);
}

int sae_dropout_advance(void* stream, uint64_t* rng, uint64_t n) {
  if (!rng) return fail(SAE_EINVAL, "dropout: rng must be non-NULL");
  return launch("dropout_advance", dropout_advance_kernel, 1LL, dim3(64), 0, (hipStream_t)stream,
                reinterpret_cast<unsigned long long*>(rng), (unsigned long long)n);
}

// ------------------------------------------------------------------------- relative logits
int sae_relpos_bias_fwd(void* stream, int32_t B, int32_t H, int32_t Hs, int32_t Ws, int32_t D, int32_t dtype,
                        const void* qhat, const int64_t qs[3], const float* eh, const float* ew, float* bias_h,
                        float* bias_w) {
  int rc = rel_validate(B, H, Hs, Ws, D, dtype);
  if (rc) return rc;
  if (!qhat || !qs || !eh || !ew || !bias_h || !bias_w) return fail(SAE_EINVAL, "NULL argument");
  RelArgs a;
  memset(&a, 0, sizeof a);
  a.qhat = qhat;
  for (int i = 0; i < 3; ++i) a.qs[i] = qs[i];
  a.eh = eh;
  a.ew = ew;
  a.bias_h = bias_h;
  a.bias_w = bias_w;
  a.B = B;
  a.H = H;
  a.Hs = Hs;
  a.Ws = Ws;
  a.D = D;
  const long long n = (long long)B * H * Hs * Ws * (Hs + Ws);
  return launch("relpos_bias_fwd", dtype == SAE_DTYPE_BF16 ? relpos_bias_fwd_kernel<__bf16> : relpos_bias_fwd_kernel<float>,
                blocks256(n), dim3(256), 0, (hipStream_t)stream, a);
}

size_t sae_relpos_bias_bwd_workspace_bytes(int32_t B, int32_t Hs, int32_t Ws, int32_t D) {
  if (B < 1 || Hs < 1 || Ws < 1 || D < 1) return 0;
  return (((size_t)B * ((2 * Hs - 1) + (2 * Ws - 1)) * D * sizeof(float)) + 255) & ~(size_t)255;
}

int sae_relpos_bias_bwd(void* stream, int32_t B, int32_t H, int32_t Hs, int32_t Ws, int32_t D, int32_t dtype,
                        const void* qhat, const int64_t qs[3], const float* eh, const float* ew,
                        const float* dbias_h, const float* dbias_w, const void* dq_in, void* dq_out,
                        const int64_t dqs[3], float* demb_h, float* demb_w, void* workspace) {
  int rc = rel_validate(B, H, Hs, Ws, D, dtype);
  if (rc) return rc;
  if (!qhat || !qs || !eh || !ew || !dbias_h || !dbias_w || !dq_out || !dqs || !demb_h || !demb_w || !workspace)
    return fail(SAE_EINVAL, "NULL argument");
  RelArgs a;
  memset(&a, 0, sizeof a);
  a.qhat = qhat;
  for (int i = 0; i < 3; ++i) {
    a.qs[i] = qs[i];
    a.dqs[i] = dqs[i];
  }
  a.eh = eh;
  a.ew = ew;
  a.dbias_h = dbias_h;
  a.dbias_w = dbias_w;
  a.dq_in = dq_in;
  a.dq_out = dq_out;
  a.demb_h = demb_h;
  a.demb_w = demb_w;
  a.part = reinterpret_cast<float*>(workspace);
  a.B = B;
  a.H = H;
  a.Hs = Hs;
  a.Ws = Ws;
  a.D = D;
  hipStream_t st = (hipStream_t)stream;
  const long long n1 = (long long)B * Hs * Ws * H * D;
  const long long n2 = (long long)B * ((2 * Hs - 1) + (2 * Ws - 1)) * D;
  const long long n3 = (long long)((2 * Hs - 1) + (2 * Ws - 1)) * D;
  const bool bf = dtype == SAE_DTYPE_BF16;
  if (int rc2 = launch("relpos_bias_bwd_dq", bf ? relpos_bias_bwd_dq_kernel<__bf16> : relpos_bias_bwd_dq_kernel<float>,
                       blocks256(n1), dim3(256), 0, st, a))
    return rc2;
  if (int rc2 = launch("relpos_bias_bwd_emb_partial",
                       bf ? relpos_bias_bwd_emb_partial_kernel<__bf16> : relpos_bias_bwd_emb_partial_kernel<float>,
                       blocks256(n2), dim3(256), 0, st, a))
    return rc2;
  return launch("relpos_bias_bwd", relpos_bias_bwd_emb_reduce_kernel, blocks256(n3), dim3(256), 0, st, a);
}

// ---------------------------------------------------------------------------------- rotary
int sae_rotary(void* stream, int32_t B, int32_t N, int32_t H, int32_t D, int32_t dtype, const void* x,
               const int64_t xs[3], void* y, const int64_t ys[3], const float* sin_t, const float* cos_t,
               int32_t inverse) {
  if (B < 1 || N < 1 || H < 1 || D < 2 || (D & 1)) return fail(SAE_EINVAL, "rotary needs sizes >= 1 and even D");
  if (dtype != SAE_DTYPE_BF16 && dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "bad dtype %d", dtype);
  if (!x || !xs || !y || !ys || !sin_t || !cos_t) return fail(SAE_EINVAL, "NULL argument");
  RotArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.y = y;
  for (int i = 0; i < 3; ++i) {
    a.xs[i] = xs[i];
    a.ys[i] = ys[i];
  }
  a.sin_t = sin_t;
  a.cos_t = cos_t;
  a.B = B;
  a.N = N;
  a.H = H;
  a.D = D;
  a.sgn = inverse ? -1.f : 1.f;
  const long long n = (long long)B * N * H * (D / 2);
  return launch("rotary", dtype == SAE_DTYPE_BF16 ? rotary_kernel<__bf16> : rotary_kernel<float>, blocks256(n),
                dim3(256), 0, (hipStream_t)stream, a);
}

#ifdef SAE_STAMPS
// diagnostic build only (not declared in sae_attn.h): copy / clear the in-kernel stamp table.  The
// table is per translation unit (common.h); this is the one of the stamped kernels (fwd2.h, bwd2.h,
// bwd3.h as instantiated here; the AGPR unit's instances write a table nobody reads).
int sae_dev_stamps(void* dst, size_t bytes, int clear) {
  if (bytes > sizeof(unsigned long long) * (size_t)kStampRecs) return fail(SAE_EINVAL, "stamps: %zu bytes", bytes);
  hipError_t e;
  e = hipDeviceSynchronize();   // every stream: no kernel may be writing stamps meanwhile
  if (e == hipSuccess && clear) {
    void* p = nullptr;
    e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_sae_stamps));
    if (e == hipSuccess) e = hipMemset(p, 0, sizeof(unsigned long long) * (size_t)kStampRecs);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  } else if (e == hipSuccess) {
    e = hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_sae_stamps), bytes, 0, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return fail(SAE_EHIP, "stamps: %s", hipGetErrorString(e));
  return ok();
}
#endif

}  // extern "C"

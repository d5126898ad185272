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

// ---------------------------------------------------------------- template dispatch helpers
template <template <typename, int, bool, bool> class L, typename... Args>
int dispatch(int dtype, int dp, bool vec, bool rel, Args&&... args) {
#define SAE_CASE(T, DPV)                                                            \
  if (dp == DPV) {                                                                  \
    if (vec) return rel ? L<T, DPV, true, true>::run(args...) : L<T, DPV, true, false>::run(args...); \
    return rel ? L<T, DPV, false, true>::run(args...) : L<T, DPV, false, false>::run(args...);        \
  }
  if (dtype == SAE_DTYPE_BF16) {
    SAE_CASE(__bf16, 32) SAE_CASE(__bf16, 64) SAE_CASE(__bf16, 128)
  } else {
    SAE_CASE(float, 32) SAE_CASE(float, 64) SAE_CASE(float, 128)
  }
#undef SAE_CASE
  return fail(SAE_EUNSUPPORTED, "no kernel instance for dtype %d dp %d", dtype, dp);
}

int rel_lds_floats(const AttnArgs& a) { return a.rel_h ? 32 * (a.rel_h + a.rel_w + 1) : 0; }

template <typename T, int DP, bool VEC, bool REL> struct FwdL {
  static int run(hipStream_t st, const AttnArgs& a) {
    const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK) + (REL ? 4 * rel_lds_floats(a) * sizeof(float) : 0);
    return launch("attn_fwd", attn_fwd_kernel<T, DP, VEC, REL>, grid, dim3(256), lds, st, a);
  }
};

template <typename T, int DP, bool VEC, bool REL> struct BwdL {
  static int run(hipStream_t st, const AttnArgs& a) {
    {  // dQ (+ delta) first: it publishes delta for the dK/dV pass
      const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
      const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK) + (REL ? 8 * rel_lds_floats(a) * sizeof(float) : 0);
      if (int rc = launch("attn_bwd_dq", attn_bwd_dq_kernel<T, DP, VEC, REL>, grid, dim3(256), lds, st, a)) return rc;
    }
    const long long grid = (long long)((a.Nk + kBKV - 1) / kBKV) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * (2 * Img<T, DP>::bytes(kBQT) + 2 * kBQT * sizeof(float) +
                                        (REL ? (size_t)kBQT * (a.rel_h + a.rel_w + 1) * sizeof(float) : 0));
    return launch("attn_bwd_dkdv", attn_bwd_dkdv_kernel<T, DP, VEC, REL>, grid, dim3(256), lds, st, a);
  }
};

// lean bf16 forward (fwd2.h): NW waves x 32 query rows per workgroup
template <int DP, int NW, int MINW, bool LSUM, bool ROT = false, int NSU = DP / 16, bool REL = false,
          bool FIX = false, bool DROP = false>
int fwd2_run(hipStream_t st, const AttnArgs& a) {
  const long long grid = (long long)((a.Nq + 32 * NW - 1) / (32 * NW)) * a.H * a.B;
  const size_t lds = 4 * (size_t)F2<DP>::TILE + (REL ? 2 * kRelImg : 0);
  return launch("attn_fwd2", attn_fwd2_kernel<DP, NW, MINW, LSUM, ROT, NSU, REL, FIX, DROP>, grid, dim3(64 * NW), lds, st, a);
}

// BoTNet relative logits on the lean bf16 kernels: the table columns (Hs + Ws) fit the two extra
// score k-steps; larger grids (up to 64 x 64) and fp32 take the v1 kernels
bool rel_lean(const AttnArgs& a) { return a.rel_h + a.rel_w <= kRelCols; }

// single query row (CaiT class attention, CeiT LCA): the K/V stream kernels of cls.h
constexpr int kClsMaxKeys = 1 << 20;
bool cls_ok(const sae_attn_desc* d) {
  return d->seq_q == 1 && d->seq_k <= kClsMaxKeys && d->head_dim <= 128 && d->dtype == SAE_DTYPE_BF16 &&
         !(d->flags & SAE_FLAG_RELPOS);
}
template <bool BWD> int cls_run(hipStream_t st, const AttnArgs& a) {
  const bool two = a.D > 64;
  const size_t lds = two ? cls_lds_bytes<2>() : cls_lds_bytes<1>();
  void (*const fn)(AttnArgs) = BWD ? (two ? attn_cls_bwd_kernel<2> : attn_cls_bwd_kernel<1>)
                                   : (two ? attn_cls_fwd_kernel<2> : attn_cls_fwd_kernel<1>);
  return launch(BWD ? "attn_cls_bwd" : "attn_cls_fwd", fn, (long long)a.B * a.H, dim3(256), lds, st, a);
}

// The lean forward's variant per padded head dim:
//   DP <= 64: three waves per SIMD, row sum on the VALU, running max fixed by the first tile (FIX,
//             with the tracking sweep as the in-kernel fallback): 23.2 vs 24.6 us at DeiT-S, 95.4 vs
//             96.5 us at ViT-B@384 (profiles/r03b_fwdvar.txt, bitwise-equal outputs).  head_dim <= 48
//             (CaiT) in 64-wide tiles without rotary: QK^T skips the all-zero fourth k-step (NSU 3).
//             The rotary instances take the same variant: the fused-rotary forward stays bit-equal
//             to the standalone rotary pass + this forward (tests/test_gpu_rotary.py).
//   DP 128:   two waves per SIMD, row sum on the MFMA (the VALU row sum is 2x slower there,
//             profiles/r01_attn_fwd_f0_vs_f6_interleaved_v13.txt).
template <int DP, bool ROT = false> int fwd2_dispatch(hipStream_t st, const AttnArgs& a) {
  if constexpr (DP <= 64) {
    if (!ROT && DP == 64 && a.D <= 48) return fwd2_run<DP, 4, 3, false, false, 3, false, true>(st, a);
    return fwd2_run<DP, 4, 3, false, ROT, DP / 16, false, true>(st, a);
  } else {
    return fwd2_run<DP, 4, 2, true, ROT>(st, a);
  }
}

// lean bf16 backward (bwd2.h): dQ pass (publishes delta) then dK/dV pass, both at two waves per SIMD
template <int DP, bool ROT = false> int bwd2_run_default(hipStream_t st, const AttnArgs& a) {
  return bwd2_run<DP, 4, 2, 4, 2, ROT>(st, a);
}

// single-pass bf16 backward (bwd3.h): one workgroup per (batch, head) holding all Nk <= 256 keys
// (8 waves x 32 keys, two waves per SIMD); longer key ranges take the two-pass bwd2
constexpr int kB3Keys = 256;

template <int DP, int NW, int KPW, bool ROT = false, int NSU = DP / 16, bool DROP = false>
int bwd3_run(hipStream_t st, const AttnArgs& a) {
  using C = B3<DP, NW, KPW>;
  static_assert(C::BK == kB3Keys, "bwd3 dispatch assumes 256-key blocks");
  if (a.Nk > C::BK) return fail(SAE_EINVAL, "bwd3: %d keys > %d", a.Nk, C::BK);
  return launch("attn_bwd3", attn_bwd3_kernel<DP, NW, KPW, ROT, NSU, DROP>, (long long)a.H * a.B, dim3(64 * NW), C::LDS, st,
                a);
}

// ------------------------------------------------------------------------------- dropout
// Attention-probability dropout (dropout.h).  The v1 kernels' DROP instances cover the whole
// envelope of the plain entry points with flags == 0 (fp32, unaligned strides or head_dim,
// head_dim > 64, a single query row).
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

// T = clamp(lrintf(rate * 256), 0, 255): a rate below 1 / 512 rounds to T = 0, no dropout
int drop_check(const sae_attn_desc* d, float rate, const uint64_t* rng, unsigned* thr) {
  if (!(rate >= 0.f && rate < 1.f)) return fail(SAE_EINVAL, "dropout rate %g is outside [0, 1)", (double)rate);
  if (!rng) return fail(SAE_EINVAL, "dropout: rng must be non-NULL");
  if (!d) return fail(SAE_EINVAL, "desc is NULL");
  if (d->flags != 0)
    return fail(SAE_EUNSUPPORTED, "dropout: flags 0x%x are not supported (no relative logits)", d->flags);
  *thr = (unsigned)std::min(255L, std::max(0L, lrintf(rate * 256.f)));
  return SAE_OK;
}

// the lean bf16 kernels' DROP instances: aligned strides, head_dim <= 64, more than one query row
bool drop_lean(const sae_attn_desc* d, bool vec, int dp) {
  return d->dtype == SAE_DTYPE_BF16 && vec && dp <= 64 && d->seq_q > 1;
}

template <typename T, int DP, bool VEC> struct FwdDropL {
  static int run(hipStream_t st, const AttnArgs& a) {
    const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK);
    return launch("attn_fwd_drop", attn_fwd_kernel<T, DP, VEC, false, true>, grid, dim3(256), lds, st, a);
  }
};

template <typename T, int DP, bool VEC> struct BwdDropL {
  static int run(hipStream_t st, const AttnArgs& a) {
    {  // dQ (+ delta) first, as in BwdL
      const long long grid = (long long)((a.Nq + kBQ - 1) / kBQ) * a.H * a.B;
      const size_t lds = nbuf<T, DP>() * 2 * Img<T, DP>::bytes(kBK);
      if (int rc = launch("attn_bwd_dq_drop", attn_bwd_dq_kernel<T, DP, VEC, false, true>, grid, dim3(256), lds, st, a))
        return rc;
    }
    const long long grid = (long long)((a.Nk + kBKV - 1) / kBKV) * a.H * a.B;
    const size_t lds = nbuf<T, DP>() * (2 * Img<T, DP>::bytes(kBQT) + 2 * kBQT * sizeof(float));
    return launch("attn_bwd_dkdv_drop", attn_bwd_dkdv_kernel<T, DP, VEC, false, true>, grid, dim3(256), lds, st, a);
  }
};

template <template <typename, int, bool> class L, typename... Args>
int dispatch_drop(int dtype, int dp, bool vec, Args&&... args) {
#define SAE_CASE(T, DPV) \
  if (dp == DPV) return vec ? L<T, DPV, true>::run(args...) : L<T, DPV, false>::run(args...);
  if (dtype == SAE_DTYPE_BF16) {
    SAE_CASE(__bf16, 32) SAE_CASE(__bf16, 64) SAE_CASE(__bf16, 128)
  } else {
    SAE_CASE(float, 32) SAE_CASE(float, 64) SAE_CASE(float, 128)
  }
#undef SAE_CASE
  return fail(SAE_EUNSUPPORTED, "no dropout kernel instance for dtype %d dp %d", dtype, dp);
}

int attn_fwd_impl(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                  const float* bias_h, const float* bias_w, void* o, float* lse, const RopeTab* rope,
                  const DropCall* drop = nullptr) {
  int rc = validate(d, false);
  if (rc) return rc;
  if (!q || !k || !v || !o) return fail(SAE_EINVAL, "q/k/v/o must be non-NULL");
  const bool rel = d->flags & SAE_FLAG_RELPOS;
  if (rel && (!bias_h || !bias_w)) return fail(SAE_EINVAL, "SAE_FLAG_RELPOS needs bias_h and bias_w");
  AttnArgs a;
  fill_args(a, d);
  a.q = q;
  a.k = k;
  a.v = v;
  a.out = o;
  a.lse = lse;
  a.bias_h = bias_h;
  a.bias_w = bias_w;
  const bool vec = desc_vec(d, {q, k, v, o}, false);
  const int var = dev_knob("SAE_FWD_VARIANT");
  hipStream_t st = (hipStream_t)stream;
  const int dp = pick_dp(d->head_dim);
  if (rope) {   // rotary rides on the lean bf16 kernels only, in the envelope of sae_attn_bwd_rotary
    if (d->dtype != SAE_DTYPE_BF16 || !vec || rel || d->flags || dp > 64)
      return fail(SAE_EUNSUPPORTED, "rotary: fused only on the bf16 path with head_dim <= 64 (16-byte aligned "
                  "strides, no flags)");
    a.rope = *rope;
    if (dp == 32) return fwd2_dispatch<32, true>(st, a);
    return fwd2_dispatch<64, true>(st, a);
  }
  if (drop) {
    fill_drop(a, *drop);
    if (drop_lean(d, vec, dp)) {
      // the lean forward's D <= 64 variant (VALU row sum, FIX) with the dropped P zeroed; at DP 64
      // the Philox state does not fit three waves per SIMD (5 / 16 VGPRs spilled): two there
      if (dp == 32) return fwd2_run<32, 4, 3, false, false, 2, false, true, true>(st, a);
      if (d->head_dim <= 48) return fwd2_run<64, 4, 2, false, false, 3, false, true, true>(st, a);
      return fwd2_run<64, 4, 2, false, false, 4, false, true, true>(st, a);
    }
    return dispatch_drop<FwdDropL>(d->dtype, dp, vec, st, a);
  }
  if (var != 1 && vec && cls_ok(d)) return cls_run<false>(st, a);
  if (var != 1 && d->dtype == SAE_DTYPE_BF16 && vec && !rel) {
    if (dp == 32) return fwd2_dispatch<32>(st, a);
    if (dp == 64) return fwd2_dispatch<64>(st, a);
    if (dp == 128) return fwd2_dispatch<128>(st, a);
  }
  if (var != 1 && d->dtype == SAE_DTYPE_BF16 && vec && rel && rel_lean(a)) {   // BoTNet
    if (dp == 32) return fwd2_run<32, 4, 2, true, false, 2, true>(st, a);
    if (dp == 64) return fwd2_run<64, 4, 2, true, false, 4, true>(st, a);
    return fwd2_run<128, 4, 2, true, false, 8, true>(st, a);
  }
  return dispatch<FwdL>(d->dtype, dp, vec, rel, st, a);
}

int attn_bwd_impl(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                  const void* o, const float* lse, const void* dout, const float* bias_h,
                  const float* bias_w, void* dq, void* dk, void* dv, float* dbias_h, float* dbias_w,
                  void* workspace, const RopeTab* rope, const DropCall* drop = nullptr) {
  int rc = validate(d, true);
  if (rc) return rc;
  if (!q || !k || !v || !o || !lse || !dout || !dq || !dk || !dv || !workspace)
    return fail(SAE_EINVAL, "q/k/v/o/lse/dout/dq/dk/dv/workspace must be non-NULL");
  const bool rel = d->flags & SAE_FLAG_RELPOS;
  if (rel && (!bias_h || !bias_w || !dbias_h || !dbias_w))
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
  const bool vec = desc_vec(d, {q, k, v, o, dout, dq, dk, dv}, true);
  const int var = dev_knob("SAE_BWD_VARIANT");
  hipStream_t st = (hipStream_t)stream;
  const int dp = pick_dp(d->head_dim);
  if (rope) {   // rotary rides on the lean bf16 kernels only
    if (d->dtype != SAE_DTYPE_BF16 || !vec || rel || d->flags || dp > 64)
      return fail(SAE_EUNSUPPORTED, "rotary: fused only on the bf16 path with head_dim <= 64 (16-byte aligned "
                  "strides, no flags)");
    a.rope = *rope;
    if (a.Nk <= kB3Keys)
      return dp == 32 ? bwd3_run<32, 8, 1, true, 2>(st, a) : bwd3_run<64, 8, 1, true, 4>(st, a);
    return dp == 32 ? bwd2_run_default<32, true>(st, a) : bwd2_run_default<64, true>(st, a);
  }
  if (drop) {
    fill_drop(a, *drop);
    if (drop_lean(d, vec, dp)) {
      if (a.Nk <= kB3Keys) {
        if (dp == 32) return bwd3_run<32, 8, 1, false, 2, true>(st, a);
        if (d->head_dim <= 48) return bwd3_run<64, 8, 1, false, 3, true>(st, a);
        return bwd3_run<64, 8, 1, false, 4, true>(st, a);
      }
      if (dp == 32) return bwd2_run<32, 4, 2, 4, 2, false, false, true>(st, a);
      return bwd2_run<64, 4, 2, 4, 2, false, false, true>(st, a);
    }
    return dispatch_drop<BwdDropL>(d->dtype, dp, vec, st, a);
  }
  if (var != 1 && vec && cls_ok(d)) return cls_run<true>(st, a);
  if (var != 1 && d->dtype == SAE_DTYPE_BF16 && vec && !rel) {
    if (a.Nk <= kB3Keys && var != 2 && dp <= 64) {
      // (waves 4-7 staggered, the previous tile's dQ first: DeiT-S 53.6 -> 53.2 us, CaiT-S24
      // 130.7 -> 128.3 us, profiles/r06g_bwd3_stagger_ab.txt; same sums, bit-identical results)
      if (dp == 32) return bwd3_run<32, 8, 1, false, 2>(st, a);
      if (dp == 64 && d->head_dim <= 48) return bwd3_run<64, 8, 1, false, 3>(st, a);   // CaiT head_dim 48
      if (dp == 64) return bwd3_run<64, 8, 1, false, 4>(st, a);
    }
    if (dp == 32) return bwd2_run_default<32>(st, a);
    if (dp == 64) return bwd2_run_default<64>(st, a);
    // head_dim 128 (BoTNet): the dK / dV pass at one wave per SIMD (the dK / dV accumulators of 32
    // keys x 128 columns plus the K / V fragments need more than half the register file), built in
    // the AGPR translation unit (bwd_agpr.hip: accumulators in AGPRs, no spills; bot14 bwd
    // 222 -> 216 us, bot7 49 -> 47 us same box, profiles/r03f_bot_agpr_ab.txt)
    return bwd2_agpr128(st, a);
  }
  if (var != 1 && d->dtype == SAE_DTYPE_BF16 && vec && rel && rel_lean(a)) {   // BoTNet relative logits
    if (dp == 32) return bwd2_run<32, 4, 2, 4, 2, false, true>(st, a);
    if (dp == 64) return bwd2_run<64, 4, 2, 4, 1, false, true>(st, a);
    // head_dim 128 with relative logits: at 14 x 14 the dQ pass at one wave per SIMD in the AGPR
    // unit (its relative-logit state spills 75 VGPRs at two waves per SIMD): bot14+rel bwd
    // 315 -> 298 us; the 7 x 7 grid keeps the two-wave dQ pass (59 vs 67 us).  The dK / dV pass
    // is this unit's instance at either size.
    if (a.Nk < 128) return bwd2_run<128, 4, 2, 4, 1, false, true>(st, a);
    if (int rc2 = bwd2_agpr128_rel_dq(st, a)) return rc2;
    return bwd2_dkdv_run<128, 4, 1, false, true>(st, a);
  }
  return dispatch<BwdL>(d->dtype, dp, vec, rel, st, a);
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

// th.hip -- the talking-heads attention entry points of the C ABI (th_kernels.h: fp32 / unaligned;
// th2.h: bf16 with the head mixes on the MFMA).
#include "th_kernels.h"
#include "th2.h"
#include "desc.h"

using namespace sae;

namespace {

// query / key blocks of 32 rows per batch entry; one wave per head (or per HPW heads)
long long th_blocks(int n, int B) { return (long long)((n + 31) / 32) * B; }

template <typename T, int DP, bool VEC> int th_fwd_run(hipStream_t st, const ThArgs& a) {
  size_t lds = kTabBytes + 2 * (size_t)a.H * 4096 + (sizeof(T) == 2 ? (size_t)a.H * Img<T, DP>::bytes(32) : 0);
  return launch("th_fwd", th_fwd_kernel<T, DP, VEC>, th_blocks(a.Nq, a.B), dim3(64 * a.H), lds, st, a);
}

int th_reduce(hipStream_t st, const ThArgs& a) {
  return launch("th_reduce", th_reduce_kernel, (long long)2 * a.H * a.H, dim3(256), 0, st, a);
}

template <typename T, int DP, bool VEC> int th_bwd_run(hipStream_t st, ThArgs a) {
  a.nblk = (int)th_blocks(a.Nq, a.B);
  size_t lds_q = kTabBytes + 2 * (size_t)a.H * 4096 + (size_t)a.H * 2 * a.H * 64 * sizeof(float) +
                 (sizeof(T) == 2 ? (size_t)a.H * Img<T, DP>::bytes(32) : 0);
  if (int rc = launch("th_bwd_q", th_bwd_q_kernel<T, DP, VEC>, th_blocks(a.Nq, a.B), dim3(64 * a.H), lds_q, st, a))
    return rc;
  size_t lds_kv = kTabBytes + 2 * (size_t)a.H * 4096 + (size_t)a.H * 64 * sizeof(float) +
                  (sizeof(T) == 2 ? (size_t)a.H * 2 * Img<T, DP>::bytes(32) : 0);
  if (int rc = launch("th_bwd_kv", th_bwd_kv_kernel<T, DP, VEC>, th_blocks(a.Nk, a.B), dim3(64 * a.H), lds_kv, st, a))
    return rc;
  return th_reduce(st, a);
}

// bf16 with the head mixes on the MFMA (th2.h).  H <= 8: one wave per head (NWMAX 8).  9..16 heads:
// two heads per wave (eight waves of <= 256 registers; sixteen waves of 128 spilled heavily).
template <int DP, int NWMAX, bool ROT, int HPW, bool LEAN = false, int NSU = DP / 16>
int th2_fwd_run(hipStream_t st, const ThArgs& a) {
  const int nw = (a.H + HPW - 1) / HPW;
  const size_t lds = th2_lds_bytes<DP, NWMAX * HPW <= 8>(a.H, 1, LEAN);
  return launch("th2_fwd", th2_fwd_kernel<DP, NWMAX, ROT, HPW, LEAN, NSU>, th_blocks(a.Nq, a.B), dim3(64 * nw), lds, st,
                a);
}

// LEAN: the query pass at two workgroups per CU (the key pass LEAN -- K / V / Q / dO re-read per
// query tile, 13 spilled registers -- measured 306 vs 230 us: profiles/r06t_th_kv_lean_rejected.txt)
template <int DP, int NWMAX, bool ROT, int HPW, bool LEAN = false, int NSU = DP / 16>
int th2_bwd_run(hipStream_t st, ThArgs a) {
  constexpr bool KST = NWMAX * HPW <= 8;
  const int nw = (a.H + HPW - 1) / HPW;
  a.nblk = (int)th_blocks(a.Nq, a.B);
  const size_t lds = th2_lds_bytes<DP, KST>(a.H, LEAN ? 2 : HPW);
  const size_t lds_kv = th2_kv_lds_bytes<DP, KST>(a.H, KST && HPW == 1);
  if (int rc = launch("th2_bwd_q", th2_bwd_q_kernel<DP, NWMAX, ROT, HPW, LEAN, NSU>, th_blocks(a.Nq, a.B),
                      dim3(64 * nw), lds, st, a))
    return rc;
  if (int rc = launch("th2_bwd_kv", th2_bwd_kv_kernel<DP, NWMAX, ROT, HPW>, th_blocks(a.Nk, a.B), dim3(64 * nw), lds_kv,
                      st, a))
    return rc;
  return th_reduce(st, a);
}

// <= 8 heads: the forward at <= 128 VGPRs, two workgroups per CU (CaiT-S24 207 -> 184 us,
// profiles/r05v_th_lean_ab.txt)
// round 6, DP 64 at D <= 48 (every CaiT width): three head-dim k-steps (NSU 3) -- the forward fits
// 128 VGPRs without spills (its scratch traffic was 1.4x the algorithmic bytes: 172 -> 160 us at
// CaiT-S24, 1.05x; profiles/r06s_th_lean_ab.txt)
template <int DP> int th2_fwd_dispatch(hipStream_t st, const ThArgs& a) {
  if constexpr (DP == 64)
    if (a.H <= 8 && a.D <= 48)
      return a.rope.sin ? th2_fwd_run<64, 8, true, 1, true, 3>(st, a) : th2_fwd_run<64, 8, false, 1, true, 3>(st, a);
  if (a.rope.sin) return a.H <= 8 ? th2_fwd_run<DP, 8, true, 1, true>(st, a) : th2_fwd_run<DP, 8, true, 2>(st, a);
  return a.H <= 8 ? th2_fwd_run<DP, 8, false, 1, true>(st, a) : th2_fwd_run<DP, 8, false, 2>(st, a);
}
// round 6: the query pass LEAN (two workgroups per CU) at <= 8 heads without rotary (CaiT-S24
// backward 540 -> 474 us; profiles/r06s_th_lean_ab.txt)
template <int DP> int th2_bwd_dispatch(hipStream_t st, const ThArgs& a) {
  if constexpr (DP == 64)
    if (a.H <= 8 && !dev_knob("SAE_TH_BWDQ_WIDE")) {
      if (a.rope.sin) {
        // (rotary at D <= 48: fwd + bwd 886 -> 785 us at CaiT-S24 shape; the query pass at one
        // workgroup per CU, 210 VGPRs, 614 vs 572 us backward -- profiles/r06w_th_rotary_ab.txt)
        if (a.D <= 48) return th2_bwd_run<64, 8, true, 1, true, 3>(st, a);
      } else {
        return a.D <= 48 ? th2_bwd_run<64, 8, false, 1, true, 3>(st, a) : th2_bwd_run<64, 8, false, 1, true>(st, a);
      }
    }
  if (a.rope.sin) return a.H <= 8 ? th2_bwd_run<DP, 8, true, 1>(st, a) : th2_bwd_run<DP, 8, true, 2>(st, a);
  return a.H <= 8 ? th2_bwd_run<DP, 8, false, 1>(st, a) : th2_bwd_run<DP, 8, false, 2>(st, a);
}

// what every talking-heads entry point checks first
int th_check(const sae_attn_desc* d, bool bwd, bool have_ptrs) {
  if (int rc = validate(d, bwd)) return rc;
  if (d->flags) return fail(SAE_EINVAL, "talking heads takes no flags");
  if (!have_ptrs) return fail(SAE_EINVAL, "NULL argument");
  if (d->heads > SAE_TH_MAX_HEADS || d->head_dim > SAE_TH_MAX_HEAD_DIM)
    return fail(SAE_EUNSUPPORTED, "talking heads needs heads <= %d and head_dim <= %d", SAE_TH_MAX_HEADS,
                SAE_TH_MAX_HEAD_DIM);
  return SAE_OK;
}

// the fp32 / unaligned kernels (th_kernels.h) take neither rotary nor more than kThMaxH heads
int th_v1_check(const sae_attn_desc* d, const RopeTab* rope) {
  if (rope) return fail(SAE_EUNSUPPORTED, "rotary: fused only on the bf16 talking-heads path (aligned strides)");
  if (d->heads > kThMaxH) return fail(SAE_EUNSUPPORTED, "talking heads: %d heads > %d on the fp32 / unaligned path",
                                      d->heads, kThMaxH);
  return SAE_OK;
}

int th_fwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v, const float* th1,
           const float* th2, void* o, float* lse, const RopeTab* rope) {
  ThArgs a;
  fill_desc(a, d);
  if (rope) a.rope = *rope;
  a.q = q;
  a.k = k;
  a.v = v;
  a.o = o;
  a.lse = lse;
  a.th1 = th1;
  a.th2 = th2;
  const bool vec = desc_vec(d, {q, k, v, o}, false);
  hipStream_t st = (hipStream_t)stream;
  const int dp = pick_dp(d->head_dim);
  if (d->dtype == SAE_DTYPE_BF16 && vec) {   // head mixes on the matrix pipe
    if (dp == 32) return th2_fwd_dispatch<32>(st, a);
    if (dp == 64) return th2_fwd_dispatch<64>(st, a);
  }
  if (int rc = th_v1_check(d, rope)) return rc;
#define TH_F(T, DPV) \
  if (dp == DPV) return vec ? th_fwd_run<T, DPV, true>(st, a) : th_fwd_run<T, DPV, false>(st, a);
  if (d->dtype == SAE_DTYPE_BF16) {
    TH_F(__bf16, 32) TH_F(__bf16, 64)
  } else {
    TH_F(float, 32) TH_F(float, 64)
  }
#undef TH_F
  return fail(SAE_EUNSUPPORTED, "talking heads: no kernel for dtype %d head_dim %d", d->dtype, d->head_dim);
}

int th_bwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v, const float* th1,
           const float* th2, const float* lse, const void* dout, void* dq, void* dk, void* dv, float* dth1,
           float* dth2, void* workspace, const RopeTab* rope) {
  ThArgs a;
  fill_desc(a, d);
  if (rope) a.rope = *rope;
  a.q = q;
  a.k = k;
  a.v = v;
  a.lse = const_cast<float*>(lse);
  a.dout = dout;
  a.dq = dq;
  a.dk = dk;
  a.dv = dv;
  a.th1 = th1;
  a.th2 = th2;
  a.dth1 = dth1;
  a.dth2 = dth2;
  a.delta = reinterpret_cast<float*>(workspace);
  a.part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + delta_bytes(d));
  const bool vec = desc_vec(d, {q, k, v, dout, dq, dk, dv}, true);
  hipStream_t st = (hipStream_t)stream;
  const int dp = pick_dp(d->head_dim);
  if (d->dtype == SAE_DTYPE_BF16 && vec) {
    if (dp == 32) return th2_bwd_dispatch<32>(st, a);
    if (dp == 64) return th2_bwd_dispatch<64>(st, a);
  }
  if (int rc = th_v1_check(d, rope)) return rc;
#define TH_B(T, DPV) \
  if (dp == DPV) return vec ? th_bwd_run<T, DPV, true>(st, a) : th_bwd_run<T, DPV, false>(st, a);
  if (d->dtype == SAE_DTYPE_BF16) {
    TH_B(__bf16, 32) TH_B(__bf16, 64)
  } else {
    TH_B(float, 32) TH_B(float, 64)
  }
#undef TH_B
  return fail(SAE_EUNSUPPORTED, "talking heads: no kernel for dtype %d head_dim %d", d->dtype, d->head_dim);
}

}  // namespace

extern "C" {

int sae_th_attn_fwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                    const float* th1, const float* th2, void* o, float* lse) {
  if (int rc = th_check(d, false, q && k && v && th1 && th2 && o && lse)) return rc;
  return th_fwd(stream, d, q, k, v, th1, th2, o, lse, nullptr);
}

size_t sae_th_attn_bwd_workspace_bytes(const sae_attn_desc* d) {
  if (!d) return 0;
  const size_t part = (size_t)th_blocks(d->seq_q, d->batch) * 2 * d->heads * d->heads * sizeof(float);
  return delta_bytes(d) + ((part + 255) & ~(size_t)255);
}

int sae_th_attn_bwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                    const float* th1, const float* th2, const float* lse, const void* dout, void* dq, void* dk,
                    void* dv, float* dth1, float* dth2, void* workspace) {
  if (int rc = th_check(d, true, q && k && v && th1 && th2 && lse && dout && dq && dk && dv && dth1 && dth2 && workspace))
    return rc;
  return th_bwd(stream, d, q, k, v, th1, th2, lse, dout, dq, dk, dv, dth1, dth2, workspace, nullptr);
}

int sae_th_attn_fwd_rotary(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                           const float* th1, const float* th2, const float* sin_tab, const float* cos_tab, void* o,
                           float* lse) {
  if (int rc = th_check(d, false, q && k && v && th1 && th2 && o && lse)) return rc;
  if (int rc = rope_check(d, sin_tab, cos_tab)) return rc;
  const RopeTab t = make_rope(d, sin_tab, cos_tab);
  return th_fwd(stream, d, q, k, v, th1, th2, o, lse, &t);
}

int sae_th_attn_bwd_rotary(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                           const float* th1, const float* th2, const float* lse, const void* dout,
                           const float* sin_tab, const float* cos_tab, void* dq, void* dk, void* dv, float* dth1,
                           float* dth2, void* workspace) {
  if (int rc = th_check(d, true, q && k && v && th1 && th2 && lse && dout && dq && dk && dv && dth1 && dth2 && workspace))
    return rc;
  if (int rc = rope_check(d, sin_tab, cos_tab)) return rc;
  const RopeTab t = make_rope(d, sin_tab, cos_tab);
  return th_bwd(stream, d, q, k, v, th1, th2, lse, dout, dq, dk, dv, dth1, dth2, workspace, &t);
}

}  // extern "C"

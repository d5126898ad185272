// th.hip -- the talking-heads attention entry points of the C ABI (th_kernels.h: fp32 / unaligned;
// th2.h: bf16 with the head mixes on the MFMA).
#include "th_kernels.h"
#include "th2.h"
#include "desc.h"

using namespace sae;

namespace {

// query / key blocks of 32 rows per batch entry; one wave per head (or per HPW heads)
long long th_blocks(int n, int B) { return (long long)((n + 31) / 32) * B; }

// --------------------------------------------------------------------------- v1 launchers
// fp32 / unaligned (th_kernels.h): one instance per <T, DP, VEC>
template <typename T, int DP, bool VEC> int th_fwd_run(hipStream_t st, const ThArgs& a) {
  size_t lds = kTabBytes + 2 * (size_t)a.H * 4096 + (sizeof(T) == 2 ? (size_t)a.H * Img<T, DP>::bytes(32) : 0);
  return launch("th_fwd", th_fwd_kernel<T, DP, VEC>, th_blocks(a.Nq, a.B), dim3(64 * a.H), lds, st, a);
}

template <typename T, int DP, bool VEC> int th_bwd_q_run(hipStream_t st, const ThArgs& a) {
  size_t lds_q = kTabBytes + 2 * (size_t)a.H * 4096 + (size_t)a.H * 2 * a.H * 64 * sizeof(float) +
                 (sizeof(T) == 2 ? (size_t)a.H * Img<T, DP>::bytes(32) : 0);
  return launch("th_bwd_q", th_bwd_q_kernel<T, DP, VEC>, th_blocks(a.Nq, a.B), dim3(64 * a.H), lds_q, st, a);
}

template <typename T, int DP, bool VEC> int th_bwd_kv_run(hipStream_t st, const ThArgs& a) {
  size_t lds_kv = kTabBytes + 2 * (size_t)a.H * 4096 + (size_t)a.H * 64 * sizeof(float) +
                  (sizeof(T) == 2 ? (size_t)a.H * 2 * Img<T, DP>::bytes(32) : 0);
  return launch("th_bwd_kv", th_bwd_kv_kernel<T, DP, VEC>, th_blocks(a.Nk, a.B), dim3(64 * a.H), lds_kv, st, a);
}

// dT1 / dT2: fixed-order sum of the query pass's per-block partials (both paths)
int th_reduce(hipStream_t st, const ThArgs& a) {
  return launch("th_reduce", th_reduce_kernel, (long long)2 * a.H * a.H, dim3(256), 0, st, a);
}

// -------------------------------------------------------------------------- th2 launchers
// bf16 with the head mixes on the MFMA (th2.h).  H <= 8: one wave per head (NWMAX 8).  9..16 heads:
// two heads per wave (eight waves of <= 256 registers; sixteen waves of 128 spilled heavily).
template <int DP, int NWMAX, bool ROT, int HPW, bool LEAN, int NSU>
int th2_fwd_run(hipStream_t st, const ThArgs& a) {
  const int nw = (a.H + HPW - 1) / HPW;
  const size_t lds = th2_lds_bytes<DP, NWMAX * HPW <= 8>(a.H, 1, LEAN);
  return launch("th2_fwd", th2_fwd_kernel<DP, NWMAX, ROT, HPW, LEAN, NSU>, th_blocks(a.Nq, a.B), dim3(64 * nw), lds, st,
                a);
}

template <int DP, int NWMAX, bool ROT, int HPW, bool LEAN, int NSU>
int th2_bwd_q_run(hipStream_t st, const ThArgs& a) {
  const int nw = (a.H + HPW - 1) / HPW;
  const size_t lds = th2_lds_bytes<DP, NWMAX * HPW <= 8>(a.H, LEAN ? 2 : HPW);
  return launch("th2_bwd_q", th2_bwd_q_kernel<DP, NWMAX, ROT, HPW, LEAN, NSU>, th_blocks(a.Nq, a.B), dim3(64 * nw), lds,
                st, a);
}

template <int DP, int NWMAX, bool ROT, int HPW> int th2_bwd_kv_run(hipStream_t st, const ThArgs& a) {
  constexpr bool KST = NWMAX * HPW <= 8;
  const int nw = (a.H + HPW - 1) / HPW;
  const size_t lds_kv = th2_kv_lds_bytes<DP, KST>(a.H, KST && HPW == 1);
  return launch("th2_bwd_kv", th2_bwd_kv_kernel<DP, NWMAX, ROT, HPW>, th_blocks(a.Nk, a.B), dim3(64 * nw), lds_kv, st,
                a);
}

// ------------------------------------------------------------------------ instance tables
// Every th2 instance is ONE row: the template parameters written once, under their names; every
// launch refers to the row's name.  `_h16` rows serve 9..16 heads (HPW 2), the others <= 8.
//
// Forward, <= 8 heads: LEAN, <= 128 VGPRs, two workgroups per CU (CaiT-S24 207 -> 184 us,
// profiles/r05v_th_lean_ab.txt).  DP 64 at D <= 48 (every CaiT width): three head-dim k-steps
// (NSU 3) -- the forward fits 128 VGPRs without spills (its scratch traffic was 1.4x the
// algorithmic bytes: 172 -> 160 us at CaiT-S24, 1.05x; profiles/r06s_th_lean_ab.txt)
//  row name               DP  NWMAX ROT    HPW LEAN   NSU
#define SAE_TH2_FWD_TABLE(X)                                  \
  X(th2_fwd_d32,           32, 8,    false, 1,  true,  2)     \
  X(th2_fwd_d32_h16,       32, 8,    false, 2,  false, 2)     \
  X(th2_fwd_d32_rot,       32, 8,    true,  1,  true,  2)     \
  X(th2_fwd_d32_rot_h16,   32, 8,    true,  2,  false, 2)     \
  X(th2_fwd_d64_k3,        64, 8,    false, 1,  true,  3)     \
  X(th2_fwd_d64,           64, 8,    false, 1,  true,  4)     \
  X(th2_fwd_d64_h16,       64, 8,    false, 2,  false, 4)     \
  X(th2_fwd_d64_rot_k3,    64, 8,    true,  1,  true,  3)     \
  X(th2_fwd_d64_rot,       64, 8,    true,  1,  true,  4)     \
  X(th2_fwd_d64_rot_h16,   64, 8,    true,  2,  false, 4)

// Backward query pass.  LEAN (two workgroups per CU) at DP 64 and <= 8 heads: without rotary
// (CaiT-S24 backward 540 -> 474 us; profiles/r06s_th_lean_ab.txt), with rotary at D <= 48 only
// (fwd + bwd 886 -> 785 us at the CaiT-S24 shape; at D 64 the query pass stays at one workgroup
// per CU, 210 VGPRs, 614 vs 572 us backward -- profiles/r06w_th_rotary_ab.txt).  The key pass LEAN
// -- K / V / Q / dO re-read per query tile, 13 spilled registers -- measured 306 vs 230 us:
// profiles/r06t_th_kv_lean_rejected.txt.
//  row name                   DP  NWMAX ROT    HPW LEAN   NSU
#define SAE_TH2_BWD_Q_TABLE(X)                                    \
  X(th2_bwd_q_d32,             32, 8,    false, 1,  false, 2)     \
  X(th2_bwd_q_d32_h16,         32, 8,    false, 2,  false, 2)     \
  X(th2_bwd_q_d32_rot,         32, 8,    true,  1,  false, 2)     \
  X(th2_bwd_q_d32_rot_h16,     32, 8,    true,  2,  false, 2)     \
  X(th2_bwd_q_d64_lean_k3,     64, 8,    false, 1,  true,  3)     \
  X(th2_bwd_q_d64_lean,        64, 8,    false, 1,  true,  4)     \
  X(th2_bwd_q_d64_rot_lean_k3, 64, 8,    true,  1,  true,  3)     \
  X(th2_bwd_q_d64,             64, 8,    false, 1,  false, 4)     \
  X(th2_bwd_q_d64_h16,         64, 8,    false, 2,  false, 4)     \
  X(th2_bwd_q_d64_rot,         64, 8,    true,  1,  false, 4)     \
  X(th2_bwd_q_d64_rot_h16,     64, 8,    true,  2,  false, 4)

//  row name               DP  NWMAX ROT    HPW
#define SAE_TH2_BWD_KV_TABLE(X)                 \
  X(th2_bwd_kv_d32,         32, 8,    false, 1)  \
  X(th2_bwd_kv_d32_h16,     32, 8,    false, 2)  \
  X(th2_bwd_kv_d32_rot,     32, 8,    true,  1)  \
  X(th2_bwd_kv_d32_rot_h16, 32, 8,    true,  2)  \
  X(th2_bwd_kv_d64,         64, 8,    false, 1)  \
  X(th2_bwd_kv_d64_h16,     64, 8,    false, 2)  \
  X(th2_bwd_kv_d64_rot,     64, 8,    true,  1)  \
  X(th2_bwd_kv_d64_rot_h16, 64, 8,    true,  2)

// one launch of a route: a table row, a v1 launcher or the reduce
#define SAE_ROW(name, ...) name,
enum class Inst {
  SAE_TH2_FWD_TABLE(SAE_ROW) SAE_TH2_BWD_Q_TABLE(SAE_ROW) SAE_TH2_BWD_KV_TABLE(SAE_ROW)
  th_fwd,   // the three v1 launchers, in the order th_v1_run indexes them
  th_bwd_q,
  th_bwd_kv,
  th_reduce,
};
#undef SAE_ROW

const char* inst_name(Inst i) {
  switch (i) {
#define SAE_ROW(name, ...) \
  case Inst::name: return #name;
    SAE_TH2_FWD_TABLE(SAE_ROW) SAE_TH2_BWD_Q_TABLE(SAE_ROW) SAE_TH2_BWD_KV_TABLE(SAE_ROW)
#undef SAE_ROW
    case Inst::th_fwd: return "th_fwd";
    case Inst::th_bwd_q: return "th_bwd_q";
    case Inst::th_bwd_kv: return "th_bwd_kv";
    case Inst::th_reduce: return "th_reduce";
  }
  return "?";
}

struct ThV1 {
  int dtype, dp;
  bool vec;
};

template <typename T> int th_v1_run(Inst i, const ThV1& v, hipStream_t st, const ThArgs& a) {
  using Fn = int (*)(hipStream_t, const ThArgs&);
#define SAE_V1(run) {{run<T, 32, false>, run<T, 32, true>}, {run<T, 64, false>, run<T, 64, true>}}
  static const Fn fn[3][2][2] = {SAE_V1(th_fwd_run), SAE_V1(th_bwd_q_run), SAE_V1(th_bwd_kv_run)};
#undef SAE_V1
  return fn[(int)i - (int)Inst::th_fwd][v.dp == 64][v.vec](st, a);
}

int run_inst(Inst i, const ThV1& v1, hipStream_t st, const ThArgs& a) {
  switch (i) {
#define SAE_F(name, ...) \
  case Inst::name: return th2_fwd_run<__VA_ARGS__>(st, a);
#define SAE_Q(name, ...) \
  case Inst::name: return th2_bwd_q_run<__VA_ARGS__>(st, a);
#define SAE_KV(name, ...) \
  case Inst::name: return th2_bwd_kv_run<__VA_ARGS__>(st, a);
    SAE_TH2_FWD_TABLE(SAE_F) SAE_TH2_BWD_Q_TABLE(SAE_Q) SAE_TH2_BWD_KV_TABLE(SAE_KV)
#undef SAE_F
#undef SAE_Q
#undef SAE_KV
    case Inst::th_fwd:
    case Inst::th_bwd_q:
    case Inst::th_bwd_kv:
      return v1.dtype == SAE_DTYPE_BF16 ? th_v1_run<__bf16>(i, v1, st, a) : th_v1_run<float>(i, v1, st, a);
    case Inst::th_reduce: return th_reduce(st, a);
  }
  return fail(SAE_EINVAL, "talking heads: bad instance %d", (int)i);
}

// ------------------------------------------------------------------------------- the plan
// The one routing decision of the talking-heads entry points: sae_th_attn_route reports it, the
// entry points launch it.  Pure: no HIP call, no pointer; the caller reads the dev knob.
struct ThFacts {
  int pass, form;   // SAE_PASS_*, SAE_FORM_*
  int dtype, D, dp, H;
  bool vec;         // desc_vec: 16-byte aligned strides, head_dim and pointers
  int wide;         // SAE_TH_BWDQ_WIDE: the query pass never LEAN
};

struct ThPlan {
  int n;
  Inst step[3];
  ThV1 v1;   // the v1 steps' instance
};

int route(ThPlan* p, Inst s0) {
  p->n = 1;
  p->step[0] = s0;
  return SAE_OK;
}
int route(ThPlan* p, Inst q, Inst kv) {   // every backward ends in the reduce
  p->n = 3;
  p->step[0] = q;
  p->step[1] = kv;
  p->step[2] = Inst::th_reduce;
  return SAE_OK;
}

int th_plan(const ThFacts& f, ThPlan* p) {
  using I = Inst;
  if (f.form == SAE_FORM_DROPOUT) return fail(SAE_EUNSUPPORTED, "talking heads has no dropout form");
  const bool bwd = f.pass == SAE_PASS_BWD, rot = f.form == SAE_FORM_ROTARY;
  const bool d64 = f.dp == 64, h16 = f.H > 8, k3 = d64 && f.D <= 48;
  p->v1 = ThV1{f.dtype, f.dp, f.vec};
  if (f.dtype == SAE_DTYPE_BF16 && f.vec && (f.dp == 32 || d64)) {   // head mixes on the matrix pipe
    // rows by [DP 64][rotary][9..16 heads]
    static const I fwd[2][2][2] = {{{I::th2_fwd_d32, I::th2_fwd_d32_h16}, {I::th2_fwd_d32_rot, I::th2_fwd_d32_rot_h16}},
                                   {{I::th2_fwd_d64, I::th2_fwd_d64_h16}, {I::th2_fwd_d64_rot, I::th2_fwd_d64_rot_h16}}};
    static const I bq[2][2][2] = {
        {{I::th2_bwd_q_d32, I::th2_bwd_q_d32_h16}, {I::th2_bwd_q_d32_rot, I::th2_bwd_q_d32_rot_h16}},
        {{I::th2_bwd_q_d64, I::th2_bwd_q_d64_h16}, {I::th2_bwd_q_d64_rot, I::th2_bwd_q_d64_rot_h16}}};
    static const I bkv[2][2][2] = {
        {{I::th2_bwd_kv_d32, I::th2_bwd_kv_d32_h16}, {I::th2_bwd_kv_d32_rot, I::th2_bwd_kv_d32_rot_h16}},
        {{I::th2_bwd_kv_d64, I::th2_bwd_kv_d64_h16}, {I::th2_bwd_kv_d64_rot, I::th2_bwd_kv_d64_rot_h16}}};
    if (!bwd) {
      if (k3 && !h16) return route(p, rot ? I::th2_fwd_d64_rot_k3 : I::th2_fwd_d64_k3);
      return route(p, fwd[d64][rot][h16]);
    }
    I q = bq[d64][rot][h16];
    if (d64 && !h16 && !f.wide) {
      if (!rot) q = k3 ? I::th2_bwd_q_d64_lean_k3 : I::th2_bwd_q_d64_lean;
      else if (k3) q = I::th2_bwd_q_d64_rot_lean_k3;
    }
    return route(p, q, bkv[d64][rot][h16]);
  }
  // the fp32 / unaligned kernels (th_kernels.h) take neither rotary nor more than kThMaxH heads
  if (rot) return fail(SAE_EUNSUPPORTED, "rotary: fused only on the bf16 talking-heads path (aligned strides)");
  if (f.H > kThMaxH)
    return fail(SAE_EUNSUPPORTED, "talking heads: %d heads > %d on the fp32 / unaligned path", f.H, kThMaxH);
  if (f.dp != 32 && !d64)
    return fail(SAE_EUNSUPPORTED, "talking heads: no kernel for dtype %d head_dim %d", f.dtype, f.D);
  return bwd ? route(p, I::th_bwd_q, I::th_bwd_kv) : route(p, I::th_fwd);
}

ThFacts th_facts(const sae_attn_desc* d, int pass, int form, bool vec) {
  return ThFacts{pass, form, d->dtype, d->head_dim, pick_dp(d->head_dim), d->heads, vec, dev_knob("SAE_TH_BWDQ_WIDE")};
}

int run_plan(const ThPlan& p, hipStream_t st, const ThArgs& a) {
  for (int i = 0; i < p.n; ++i)
    if (int rc = run_inst(p.step[i], p.v1, st, a)) return rc;
  return SAE_OK;
}

// the route's name: its launches in order, the v1 steps with their instance
std::string plan_name(const ThPlan& p) {
  std::string s;
  for (int i = 0; i < p.n; ++i) {
    s += i ? "+" : "";
    s += inst_name(p.step[i]);
    if (p.step[i] == Inst::th_fwd || p.step[i] == Inst::th_bwd_q || p.step[i] == Inst::th_bwd_kv)
      s += std::string(p.v1.dtype == SAE_DTYPE_BF16 ? "_bf16_d" : "_f32_d") + std::to_string(p.v1.dp) +
           (p.v1.vec ? "" : "_scalar");
  }
  return s;
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

// ------------------------------------------------------ entry points: check, fill, plan, launch
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
  ThPlan p;
  const int form = rope ? SAE_FORM_ROTARY : SAE_FORM_PLAIN;
  if (int rc = th_plan(th_facts(d, SAE_PASS_FWD, form, desc_vec(d, {q, k, v, o}, false)), &p)) return rc;
  return run_plan(p, (hipStream_t)stream, a);
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
  a.nblk = (int)th_blocks(a.Nq, a.B);
  ThPlan p;
  const int form = rope ? SAE_FORM_ROTARY : SAE_FORM_PLAIN;
  if (int rc = th_plan(th_facts(d, SAE_PASS_BWD, form, desc_vec(d, {q, k, v, dout, dq, dk, dv}, true)), &p)) return rc;
  return run_plan(p, (hipStream_t)stream, a);
}

}  // namespace

extern "C" {

int sae_th_attn_fwd(void* stream, const sae_attn_desc* d, const void* q, const void* k, const void* v,
                    const float* th1, const float* th2, void* o, float* lse) {
  if (int rc = th_check(d, false, q && k && v && th1 && th2 && o && lse)) return rc;
  return th_fwd(stream, d, q, k, v, th1, th2, o, lse, nullptr);
}

// host-only: the plan of the entry point of that pass and form, by name (no HIP call)
const char* sae_th_attn_route(const sae_attn_desc* d, int32_t pass, int32_t form, int32_t aligned) {
  static thread_local std::string name;
  if (route_args_check(pass, form)) return nullptr;
  const bool bwd = pass == SAE_PASS_BWD;
  if (th_check(d, bwd, true)) return nullptr;
  if (form == SAE_FORM_ROTARY && rope_dim_check(d)) return nullptr;
  ThPlan p;
  if (th_plan(th_facts(d, pass, form, aligned && desc_strides_vec(d, bwd)), &p)) return nullptr;
  name = plan_name(p);
  ok();
  return name.c_str();
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

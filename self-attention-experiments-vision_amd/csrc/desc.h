// desc.h -- host side of sae_attn_desc, shared by the attention and the talking-heads units:
// validation, the descriptor -> kernel-argument copy, the 16-byte vector predicate, the delta
// workspace size and the rotary-table argument.
#pragma once
#include "common.h"
#include "host.h"

namespace sae {

inline int validate(const sae_attn_desc* d, bool bwd) {
  if (!d) return fail(SAE_EINVAL, "desc is NULL");
  if (d->batch < 1 || d->heads < 1 || d->seq_q < 1 || d->seq_k < 1 || d->head_dim < 1)
    return fail(SAE_EINVAL, "batch/heads/seq_q/seq_k/head_dim must be >= 1 (got %d/%d/%d/%d/%d)", d->batch,
                d->heads, d->seq_q, d->seq_k, d->head_dim);
  if (d->dtype != SAE_DTYPE_BF16 && d->dtype != SAE_DTYPE_F32)
    return fail(SAE_EINVAL, "dtype %d is not SAE_DTYPE_F32 or SAE_DTYPE_BF16", d->dtype);
  if (!pick_dp(d->head_dim)) return fail(SAE_EUNSUPPORTED, "head_dim %d > 128 is not supported", d->head_dim);
  if ((d->flags & ~SAE_FLAG_RELPOS) != 0) return fail(SAE_EINVAL, "unknown flags 0x%x", d->flags);
  if (d->flags & SAE_FLAG_RELPOS) {
    if (d->rel_h < 1 || d->rel_w < 1 || d->rel_h * d->rel_w != d->seq_k)
      return fail(SAE_EINVAL, "relpos grid %dx%d does not match seq_k %d", d->rel_h, d->rel_w, d->seq_k);
    if (d->rel_w > 64 || d->rel_h > 64 || d->seq_k > 4096)
      return fail(SAE_EUNSUPPORTED, "relpos grid %dx%d exceeds 64x64", d->rel_h, d->rel_w);
  }
  if (d->seq_q > (1 << 24) || d->seq_k > (1 << 24)) return fail(SAE_EUNSUPPORTED, "sequence too long");
  if (!(d->scale > 0.f)) return fail(SAE_EINVAL, "scale must be > 0 (got %g)", (double)d->scale);
  // per-(batch, head) row ranges are addressed through 32-bit buffer descriptors
  const int es = elem_size(d->dtype);
  const int64_t* st[8] = {d->q_stride, d->k_stride, d->v_stride, d->o_stride,
                          d->do_stride, d->dq_stride, d->dk_stride, d->dv_stride};
  const char* nm[8] = {"q", "k", "v", "o", "dout", "dq", "dk", "dv"};
  for (int i = 0; i < (bwd ? 8 : 4); ++i) {
    const int64_t n = (i == 1 || i == 2 || i == 6 || i == 7) ? d->seq_k : d->seq_q;
    if (st[i][1] < d->head_dim)
      return fail(SAE_EINVAL, "%s token stride %lld < head_dim %d", nm[i], (long long)st[i][1], d->head_dim);
    if (n * st[i][1] * es >= ((int64_t)1 << 31))
      return fail(SAE_EUNSUPPORTED, "%s: %lld tokens x stride %lld exceed 32-bit row addressing", nm[i],
                  (long long)n, (long long)st[i][1]);
  }
  return SAE_OK;
}

// the fields AttnArgs and ThArgs share
template <class Args> void fill_desc(Args& a, const sae_attn_desc* d) {
  memset(&a, 0, sizeof a);
  a.B = d->batch;
  a.H = d->heads;
  a.Nq = d->seq_q;
  a.Nk = d->seq_k;
  a.D = d->head_dim;
  for (int i = 0; i < 3; ++i) {
    a.qs[i] = d->q_stride[i];
    a.ks[i] = d->k_stride[i];
    a.vs[i] = d->v_stride[i];
    a.os[i] = d->o_stride[i];
    a.dos[i] = d->do_stride[i];
    a.dqs[i] = d->dq_stride[i];
    a.dks[i] = d->dk_stride[i];
    a.dvs[i] = d->dv_stride[i];
  }
  a.scale = d->scale;
}

// 16-byte vector loads and stores: head_dim and every stride in use a whole number of 16-byte
// chunks (the descriptor's half, which the route queries share), every pointer in `ptrs` 16-byte
// aligned
inline bool desc_strides_vec(const sae_attn_desc* d, bool bwd) {
  const int epc = 16 / elem_size(d->dtype);
  bool v = d->head_dim % epc == 0 && strides_vec(d->q_stride, epc) && strides_vec(d->k_stride, epc) &&
           strides_vec(d->v_stride, epc) && strides_vec(d->o_stride, epc);
  if (bwd)
    v = v && strides_vec(d->do_stride, epc) && strides_vec(d->dq_stride, epc) && strides_vec(d->dk_stride, epc) &&
        strides_vec(d->dv_stride, epc);
  return v;
}
inline bool desc_vec(const sae_attn_desc* d, std::initializer_list<const void*> ptrs, bool bwd) {
  bool v = desc_strides_vec(d, bwd);
  for (const void* p : ptrs) v = v && aligned16(p);
  return v;
}

// pass / form of the route queries (sae_attn_route, sae_th_attn_route)
inline int route_args_check(int pass, int form) {
  if ((pass != SAE_PASS_FWD && pass != SAE_PASS_BWD) || form < SAE_FORM_PLAIN || form > SAE_FORM_DROPOUT)
    return fail(SAE_EINVAL, "route: bad pass %d or form %d", pass, form);
  return SAE_OK;
}

// delta [B, H, Nq] fp32 at the head of every backward workspace
inline size_t delta_bytes(const sae_attn_desc* d) {
  return (((size_t)d->batch * d->heads * d->seq_q * sizeof(float)) + 255) & ~(size_t)255;
}

// rotary tables of the _rotary entry points: fp32 [max(seq_q, seq_k)][head_dim / 2]
inline int rope_dim_check(const sae_attn_desc* d) {
  if (d->head_dim % 8 || d->head_dim > 64)
    return fail(SAE_EUNSUPPORTED, "rotary: fused rotary needs head_dim %% 8 == 0 and <= 64 (got %d)", d->head_dim);
  return SAE_OK;
}
inline int rope_check(const sae_attn_desc* d, const float* sin_tab, const float* cos_tab) {
  if (!sin_tab || !cos_tab) return fail(SAE_EINVAL, "rotary: sin_tab / cos_tab must be non-NULL");
  if (!aligned16(sin_tab) || !aligned16(cos_tab)) return fail(SAE_EINVAL, "rotary: tables must be 16-byte aligned");
  return rope_dim_check(d);
}
inline RopeTab make_rope(const sae_attn_desc* d, const float* sin_tab, const float* cos_tab) {
  RopeTab t;
  t.sin = sin_tab;
  t.cos = cos_tab;
  t.P = d->head_dim / 2;
  t.n = std::max(d->seq_q, d->seq_k);
  return t;
}

}  // namespace sae

/*
 * sae_attn.h -- C ABI of the MI355X (gfx950) multi-head self-attention hot path.
 *
 * This is the drop-in boundary of the build: every entry point takes plain device
 * pointers, sizes and a HIP stream (as void*), never a framework type.  It replaces the
 * XLA-lowered einsum / softmax chains of the reference's Flax attention modules
 * (cfoster0/self-attention-experiments-vision):
 *
 *   sae_attn_fwd / sae_attn_bwd
 *       AttentionBlock core, models/layers/attentions/attention.py:39-58
 *       (q/sqrt(D) :39, QK^T einsum :41-42, softmax :48, AV einsum :57-58) and its JAX
 *       autodiff backward.  Also the core of CvTAttentionBlock
 *       (models/layers/attentions/cvt_attention.py:85-104, Nq != Nk), of
 *       ClassSelfAttentionBlock (models/cait.py:10-15, Nq = 1) and of
 *       LCSelfAttentionBlock (models/ceit.py:11-16, Nq = 1).
 *   SAE_FLAG_RELPOS (bias_h / bias_w in sae_attn_fwd/bwd) + sae_relpos_bias_fwd/bwd
 *       BoTNet RelativeLogits added to the score tile, models/botnet.py:70-141,191-192.
 *   sae_th_attn_fwd / sae_th_attn_bwd
 *       talking-heads attention, attention.py:44-52 + talking_heads.py:9-14.
 *   sae_rotary
 *       rotary position embedding, models/layers/position_embed.py:8-20 (README to-do).
 *
 * Conventions
 *   - Activations are token-major [B, N, H, D] (the reference einsum layout), addressed by
 *     element strides (batch, token, head); the head_dim stride is 1.
 *   - Scores are scale * <q, k> (+ bias); the reference's scale is 1/sqrt(head_ch).
 *   - lse is float32 [B, H, Nq], the natural-log log-sum-exp of each score row.
 *   - dtype is SAE_DTYPE_BF16 (compute: bf16 MFMA, fp32 accumulate / softmax) or
 *     SAE_DTYPE_F32 (exact fp32 MFMA).
 *   - All buffers are caller-owned; nothing is allocated or retained; every launch is
 *     ordered on `stream`; no host synchronisation (graph-capturable); re-entrant.
 *   - Return 0 on success, a negative SAE_E* code otherwise; sae_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 */
#ifndef SAE_ATTN_H
#define SAE_ATTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAE_ABI_VERSION 1

enum {
  SAE_OK = 0,
  SAE_EINVAL = -1,        /* descriptor / argument validation failed */
  SAE_EUNSUPPORTED = -2,  /* valid but outside the implemented envelope (e.g. D > 128) */
  SAE_EHIP = -3           /* a HIP runtime call failed */
};

enum { SAE_DTYPE_F32 = 0, SAE_DTYPE_BF16 = 1 };

enum { SAE_FLAG_RELPOS = 1 };

typedef struct sae_attn_desc {
  int32_t batch, heads, seq_q, seq_k, head_dim;
  int32_t dtype;          /* SAE_DTYPE_* of q, k, v, o, dout, dq, dk, dv */
  int32_t flags;          /* SAE_FLAG_* */
  float scale;            /* score = scale * <q, k> + bias */
  /* element strides (batch, token, head); head_dim stride must be 1 */
  int64_t q_stride[3], k_stride[3], v_stride[3], o_stride[3];
  /* backward only */
  int64_t do_stride[3], dq_stride[3], dk_stride[3], dv_stride[3];
  /* SAE_FLAG_RELPOS: keys form a rel_h x rel_w grid (seq_k == rel_h * rel_w) and
     bias_h [B,H,Nq,rel_h], bias_w [B,H,Nq,rel_w] (fp32) are added to the scores:
     score[q, k] += bias_h[q, k / rel_w] + bias_w[q, k % rel_w]. */
  int32_t rel_h, rel_w;
} sae_attn_desc;

/* Fill `desc` for contiguous [B, N, H, D] tensors (all eight stride triples). */
void sae_attn_desc_init(sae_attn_desc* desc, int32_t batch, int32_t heads, int32_t seq_q,
                        int32_t seq_k, int32_t head_dim, int32_t dtype, float scale);

/* Forward: o = softmax(scale q k^T + bias) v, lse = logsumexp rows.
   bias_h / bias_w may be NULL unless SAE_FLAG_RELPOS.  lse may be NULL (inference). */
int sae_attn_fwd(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                 const void* v, const float* bias_h, const float* bias_w, void* o,
                 float* lse);

/* Bytes of device workspace sae_attn_bwd needs (float32 delta = rowsum(dout * o)). */
size_t sae_attn_bwd_workspace_bytes(const sae_attn_desc* desc);

/* Backward: writes dq, dk, dv (and dbias_h / dbias_w if SAE_FLAG_RELPOS: the score
   gradient summed over key rows / key columns).  Deterministic: no atomics to HBM. */
int sae_attn_bwd(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                 const void* v, const void* o, const float* lse, const void* dout,
                 const float* bias_h, const float* bias_w, void* dq, void* dk, void* dv,
                 float* dbias_h, float* dbias_w, void* workspace);

/* BoTNet relative logits (botnet.py:70-141) in index-map form, qhat = scaled query
   [B, N = Hs*Ws, H, D] (dtype), emb_h [2Hs-1, D], emb_w [2Ws-1, D] fp32:
     bias_h[b,h,n,p] = <qhat[b,n,h], emb_h[p - n/Ws + Hs - 1]>
     bias_w[b,h,n,c] = <qhat[b,n,h], emb_w[c - n%Ws + Ws - 1]>                        */
int sae_relpos_bias_fwd(void* stream, int32_t batch, int32_t heads, int32_t rel_h,
                        int32_t rel_w, int32_t head_dim, int32_t dtype, const void* qhat,
                        const int64_t qhat_stride[3], const float* emb_h,
                        const float* emb_w, float* bias_h, float* bias_w);

size_t sae_relpos_bias_bwd_workspace_bytes(int32_t batch, int32_t rel_h, int32_t rel_w,
                                           int32_t head_dim);

/* Backward of sae_relpos_bias_fwd.  dqhat_out = dqhat_in + d(bias)/d(qhat)
   (dqhat_in may equal dqhat_out, or be NULL for zero), demb_h / demb_w overwritten. */
int sae_relpos_bias_bwd(void* stream, int32_t batch, int32_t heads, int32_t rel_h,
                        int32_t rel_w, int32_t head_dim, int32_t dtype, const void* qhat,
                        const int64_t qhat_stride[3], const float* emb_h,
                        const float* emb_w, const float* dbias_h, const float* dbias_w,
                        const void* dqhat_in, void* dqhat_out, const int64_t dq_stride[3],
                        float* demb_h, float* demb_w, void* workspace);

/* Rotary embedding (position_embed.py:8-20, GPT-J interleaved pairs) on x [B,N,H,D]:
     y[2i]   = x[2i] cos[n,i] - x[2i+1] sin[n,i]
     y[2i+1] = x[2i+1] cos[n,i] + x[2i] sin[n,i]
   sin/cos are fp32 [N, D/2] tables.  inverse != 0 rotates by -theta (the backward).
   y may alias x. */
int sae_rotary(void* stream, int32_t batch, int32_t seq, int32_t heads, int32_t head_dim,
               int32_t dtype, const void* x, const int64_t x_stride[3], void* y,
               const int64_t y_stride[3], const float* sin_tab, const float* cos_tab,
               int32_t inverse);

/* Attention with the rotary embedding fused (position_embed.py:8-20 applied to q and k before
   the scores): q and k are passed UN-rotated and rotated by the kernels as they are staged
   (sin/cos fp32 [max(seq_q, seq_k)][head_dim / 2], row = position), so the rotated tensors
   never exist in memory; the backward returns dq / dk for the un-rotated q / k (rotated back
   as they are stored).  Bit-identical to sae_rotary + sae_attn_fwd / sae_attn_bwd + sae_rotary
   (inverse).  bf16, 16-byte aligned strides, head_dim % 8 == 0 and head_dim <= 64 (forward
   and backward alike, so a forward that runs always has its backward), no flags; otherwise
   SAE_EUNSUPPORTED (use sae_rotary + the plain entry points). */
int sae_attn_fwd_rotary(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                        const void* v, const float* sin_tab, const float* cos_tab, void* o,
                        float* lse);
int sae_attn_bwd_rotary(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                        const void* v, const void* o, const float* lse, const void* dout,
                        const float* sin_tab, const float* cos_tab, void* dq, void* dk, void* dv,
                        void* workspace);

/* Attention-probability dropout (attention.py:54-58: nn.Dropout(rate = attn_dropout_rate) on the
   softmax output before the AV product), regenerated from counters by forward and backward alike;
   no mask is stored, and the mask does not depend on the kernel serving the call:
     T        = clamp(lrintf(rate * 256), 0, 255),  keep probability pk = (256 - T) / 256
     (k0, k1) = words 0, 1 of Philox4x32-10(counter (lo32(offset), hi32(offset), stream_id, 0),
                                            key (lo32(seed), hi32(seed)))
     W        = Philox4x32-10(counter (k >> 2, q >> 2, b * heads + h, 0), key (k0, k1))
     keep(b, h, q, k) = ((W[q & 3] >> (8 * (k & 3))) & 0xff) >= T
     o[q] = sum_k P[q, k] * keep / pk * v[k];  lse is that of the undropped scores.
   rng points at device memory {seed, offset} (two uint64), read by the kernels, so a captured
   graph replays with a fresh mask once sae_dropout_advance has bumped the offset on the stream.
   stream_id tells the attention calls of one step apart; the backward passes the forward's.
   The rate is quantised to n / 256 and the rescale uses exactly pk; a rate below 1 / 512 gives
   T = 0, which means no dropout: the call is forwarded to sae_attn_fwd / sae_attn_bwd.
   rate outside [0, 1) or NaN, or rng == NULL: SAE_EINVAL.  desc->flags != 0: SAE_EUNSUPPORTED (no
   relative logits).  Otherwise the envelope is that of sae_attn_fwd / sae_attn_bwd. */
int sae_attn_fwd_dropout(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                         const void* v, void* o, float* lse, float rate, const uint64_t* rng,
                         uint32_t stream_id);
int sae_attn_bwd_dropout(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                         const void* v, const void* o, const float* lse, const void* dout,
                         void* dq, void* dk, void* dv,
                         void* workspace /* sae_attn_bwd_workspace_bytes */, float rate,
                         const uint64_t* rng, uint32_t stream_id);
/* keep[b][h][q][k] as uint8 0 / 1 by the definition above: what the two entry points apply. */
int sae_attn_dropout_mask(void* stream, int32_t batch, int32_t heads, int32_t seq_q, int32_t seq_k,
                          float rate, const uint64_t* rng, uint32_t stream_id, uint8_t* keep);
/* rng[1] += n on the stream (a one-thread kernel). */
int sae_dropout_advance(void* stream, uint64_t* rng, uint64_t n);

/* Hidden-state dropout (models/vit.py:12,22,29,47: nn.Dropout(rate = dropout_rate) on the encoder
   input after the position embedding, on the attention output -- attention.py out_dropout_rate --,
   on the FF hidden activation after the GELU, ff.py:30, and on the FF output, ff.py:32), on an
   activation viewed as rows x columns.  T, pk, rng = {seed, offset}, stream_id and (k0, k1) exactly
   as for the attention mask above; regenerated from counters, nothing stored, and the mask does not
   depend on the kernel applying it:
     W              = Philox4x32-10(counter (col >> 4, lo32(row), hi32(row), 1), key (k0, k1))
     keep(row, col) = ((W[(col >> 2) & 3] >> (8 * (col & 3))) & 0xff) >= T
     row            = row0 + i * row_step      (64-bit; i = the row the kernel is working on)
     y              = x * keep / pk
   One call covers 16 consecutive columns of one row; counter word 3 = 1 separates it from the
   attention mask (word 3 = 0).  row0 / row_step let a call on a strided subset of the rows (the
   class-token rows b * N) draw the mask of the full tensor.  A rate below 1 / 512 (T = 0) means no
   dropout: every entry point below then forwards to the plain one, bit-identically
   (sae_dropout_rows copies).  rate outside [0, 1) or NaN, rng == NULL, or row_step < 1: SAE_EINVAL,
   on the host before any HIP call.

   sae_dropout_rows: y = x * keep / pk on [M][C] (dtype bf16 or fp32, row strides ldx / ldy in
   elements, y may alias x); its backward is the same call on the gradient.  For the paths the
   fused forms below do not take (fp32 compute dtype, shapes outside an envelope). */
int sae_dropout_rows(void* stream, int32_t M, int32_t C, int32_t dtype, const void* x, int64_t ldx,
                     void* y, int64_t ldy, float rate, const uint64_t* rng, uint32_t stream_id,
                     int64_t row0, int64_t row_step);
/* keep[M][C] as uint8 0 / 1 by the definition above: what the other entry points apply. */
int sae_dropout_rows_mask(void* stream, int32_t M, int32_t C, float rate, const uint64_t* rng,
                          uint32_t stream_id, int64_t row0, int64_t row_step, uint8_t* keep);

/* Talking-heads attention (attention.py:41-58 with talking_heads=True):
     S = scale q k^T ; S1[i] = sum_h th1[h,i] S[h] ; P = softmax(S1) ;
     P2[i] = sum_h th2[h,i] P[h] ; o = P2 v
   th1/th2 are fp32 [H, H] ([h_in, h_out], talking_heads.py:13).  One workgroup holds one
   query (or key) block for all heads, so heads <= SAE_TH_MAX_HEADS and head_dim <=
   SAE_TH_MAX_HEAD_DIM: bf16 (16-byte aligned strides) takes up to 16 heads -- every CaiT config
   of models/create_model.py:79-168, cait_m_24/36/48 included (16 heads, head_dim 48); the fp32
   (exact) and unaligned paths take up to 8 heads.
   lse: fp32 [B, H, Nq] log-sum-exp of the mixed logits S1 (for the backward). */
#define SAE_TH_MAX_HEADS 16
#define SAE_TH_MAX_HEAD_DIM 64
int sae_th_attn_fwd(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                    const void* v, const float* th1, const float* th2, void* o, float* lse);

size_t sae_th_attn_bwd_workspace_bytes(const sae_attn_desc* desc);

/* Backward of sae_th_attn_fwd: dq, dk, dv and the transform gradients dth1, dth2
   (fp32 [H, H], overwritten; reduced deterministically through the workspace). */
int sae_th_attn_bwd(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                    const void* v, const float* th1, const float* th2, const float* lse,
                    const void* dout, void* dq, void* dk, void* dv, float* dth1,
                    float* dth2, void* workspace);

/* Talking heads with the rotary embedding fused (as sae_attn_fwd_rotary; bf16, aligned). */
int sae_th_attn_fwd_rotary(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                           const void* v, const float* th1, const float* th2,
                           const float* sin_tab, const float* cos_tab, void* o, float* lse);
int sae_th_attn_bwd_rotary(void* stream, const sae_attn_desc* desc, const void* q, const void* k,
                           const void* v, const float* th1, const float* th2, const float* lse,
                           const void* dout, const float* sin_tab, const float* cos_tab, void* dq,
                           void* dk, void* dv, float* dth1, float* dth2, void* workspace);

/* Host-only queries (no device needed, no HIP call): which kernels the attention /
   talking-heads entry point of that pass and form runs for this descriptor.  `aligned` stands for
   "every tensor pointer of the call is 16-byte aligned"; the stride half of the vector-access
   condition is read from the descriptor.  SAE_FORM_DROPOUT means a rate that drops something
   (T > 0; T = 0 is the plain form); talking heads has no dropout form.  Returns the route's name --
   the launched kernel instances in launch order, joined by '+' -- or NULL where the entry point
   would refuse the call, with the reason in sae_last_error.  The string lives until the next call
   into the library on this thread, as sae_last_error's does.  The names are the rows of the
   instance tables in csrc/attn.hip, csrc/bwd2_run.h and csrc/th.hip: informative (logs, tests),
   NOT part of the ABI -- a new kernel changes them without a new SAE_ABI_VERSION. */
#define SAE_PASS_FWD 0
#define SAE_PASS_BWD 1
#define SAE_FORM_PLAIN 0
#define SAE_FORM_ROTARY 1
#define SAE_FORM_DROPOUT 2
const char* sae_attn_route(const sae_attn_desc* desc, int32_t pass, int32_t form, int32_t aligned);
const char* sae_th_attn_route(const sae_attn_desc* desc, int32_t pass, int32_t form,
                              int32_t aligned);

/* Weight / bias gradients of a projection on the path (the Dense / DenseGeneral kernels of
   attention.py:29-37,60-63 and ff.py:8-34, whose JAX autodiff computes them):
     dw[i][j] (+)= sum_m x[m][i] * dy[m][j]      dw fp32 [I][J] (row stride ldw)
     db[j]    (+)= sum_m dy[m][j]                db fp32 [J] (may be NULL)
   x bf16 [M][I] (row stride ldx), dy bf16 [M][J] (row stride ldy); I, J, ldx, ldy multiples
   of 8, pointers 16-byte aligned.  accumulate != 0 adds into dw / db.  Split over m with a
   fixed-order reduction of the splits: deterministic, no atomics. */
size_t sae_gemm_dw_workspace_bytes(int32_t M, int32_t I, int32_t J);
int sae_gemm_dw(void* stream, int32_t M, int32_t I, int32_t J, const void* x, int64_t ldx,
                const void* dy, int64_t ldy, float* dw, int64_t ldw, float* db,
                int32_t accumulate, void* workspace);
/* Same, with dw laid out as J / jblock contiguous column blocks [J/jblock][I][jblock] (the
   separate queries / keys / values kernel gradients of one stacked projection); jblock a
   multiple of 4 dividing J.  Workspace: sae_gemm_dw_workspace_bytes(M, I, J). */
int sae_gemm_dw_blocked(void* stream, int32_t M, int32_t I, int32_t J, int32_t jblock,
                        const void* x, int64_t ldx, const void* dy, int64_t ldy, float* dw,
                        float* db, int32_t accumulate, void* workspace);

/* Forward and input-gradient GEMMs of the projections and the FF block (the dot_generals of
   Flax Dense / DenseGeneral, attention.py:29-37,60-63 and ff.py:8-34), with the FF block's
   nn.gelu (tanh form, ff.py:27) and its derivative fused into the epilogue:
     acc[m][n] = sum_k a[m][k] * bt[n][k]      a bf16 [M][K] (lda), bt bf16 [N][K] (ldb)
     SAE_EPI_NONE : c = bf16(acc + bias)
     SAE_EPI_GELU : c2 = h = bf16(acc + bias), c = bf16(gelu(h))
     SAE_EPI_DGELU: c = bf16(bf16(acc) * gelu'(aux))   (aux bf16 [M][N], ldaux; bias NULL)
     SAE_EPI_GELU_GRAD: c2 = g = bf16(gelu'(bf16(acc + bias))), c = bf16(gelu(bf16(acc + bias)))
     SAE_EPI_MUL_AUX  : c = bf16(bf16(acc) * aux)       (aux = the g above; bias NULL)
   (the FF block's pair: the forward saves gelu'(h) instead of h, so the input-gradient GEMM's
   epilogue is one multiply instead of the sigmoid algebra -- gelu' rounded to bf16 once, the
   rounding the reference's bf16 derivative carries anyway)
   c, c2 bf16 [M][N] (ldc); bias fp32 [N] or NULL.  K a multiple of 8; N, lda, ldb, ldc
   multiples of 8; pointers 16-byte aligned.  A Dense forward passes the transposed bf16
   kernel as bt (see sae_weight_cast); its input gradient passes the kernel itself. */
#define SAE_EPI_NONE 0
#define SAE_EPI_GELU 1
#define SAE_EPI_DGELU 2
#define SAE_EPI_GELU_GRAD 3
#define SAE_EPI_MUL_AUX 4
int sae_gemm_nt(void* stream, int32_t M, int32_t N, int32_t K, const void* a, int64_t lda,
                const void* bt, int64_t ldb, const float* bias, void* c, int64_t ldc,
                int32_t epilogue, const void* aux, int64_t ldaux, void* c2);
/* Which kernel sae_gemm_nt runs for a shape (host-only, no device needed): the round-5 routing
   rule by tile fill and reduction depth (gemm.hip, nt_plan: g8x_route / g8_route). */
#define SAE_NT_ROUTE_NONE 0           /* shape not supported: sae_gemm_nt returns SAE_EUNSUPPORTED */
#define SAE_NT_ROUTE_TILE128 1        /* 128-row tiles (gemm_nt_kernel), K % 64 == 0 */
#define SAE_NT_ROUTE_TILE128_KTAIL 2  /* 128-row tiles, K % 8 == 0 with a partial last K stage */
#define SAE_NT_ROUTE_GEMM8 3          /* persistent 224/256 x 192 tiles (GELU forward at K < 768: 256 x 128 where that loads the CUs more evenly), LDS-DMA (gemm8_nt_kernel) */
#define SAE_NT_ROUTE_GEMM8X 4         /* ping-pong 256 x 256 tiles, LDS-DMA (gemm8x_nt_kernel) */
int sae_gemm_nt_route(int32_t M, int32_t N, int32_t K, int32_t epilogue);
/* The same plan by name (host-only, no device needed; without one it plans for 256 compute units):
   the row of gemm.hip's instance tables that sae_gemm_nt -- dropout != 0: sae_gemm_nt_gelu_dropout,
   epilogue SAE_EPI_GELU_GRAD -- launches for the shape, e.g. "g8_192_bm224_plain"; a static string,
   or NULL with sae_last_error set.  sae_gemm_nt_instance_name(i) is row i of those tables (the image
   loaders of sae_patch_embed_fwd, "patch_*", included), NULL past the last. */
const char* sae_gemm_nt_instance(int32_t M, int32_t N, int32_t K, int32_t epilogue,
                                 int32_t dropout);
const char* sae_gemm_nt_instance_name(int32_t index);
/* The SAE_EPI_GELU_GRAD forward with the hidden dropout of ff.py:30 (the mask above over [M][N],
   row = m, col = n, row0 = 0, row_step = 1), h = bf16(acc + bias):
     c = bf16(gelu(h) * keep / pk),  c2 = bf16(gelu'(h) * keep / pk)
   each product formed in fp32 and rounded once.  The saved c2 carries the mask, so the input
   gradient is the unchanged SAE_EPI_MUL_AUX call, and sae_gemm_dw on the dropped c gives the next
   Dense's weight gradient.  Validation, shape envelope and kernel routing are those of
   sae_gemm_nt(..., SAE_EPI_GELU_GRAD, ...): sae_gemm_nt_route tells the kernel. */
int sae_gemm_nt_gelu_dropout(void* stream, int32_t M, int32_t N, int32_t K, const void* a,
                             int64_t lda, const void* bt, int64_t ldb, const float* bias, void* c,
                             int64_t ldc, void* c2, float rate, const uint64_t* rng,
                             uint32_t stream_id);
/* The same projections at compute dtype float32 (the reference's fp32 trunks, cait.py:147-154,
   and every fp32 run), on the exact-f32 MFMA:
     c[m][n] = (accumulate ? c[m][n] : 0) + sum_k A(m,k) B(k,n) (+ bias[n])
     A(m,k) = a[m*sam + k*sak], B(k,n) = b[k*sbk + n*sbn]
   One stride of each operand must be 1 (sak == 1: k-contiguous, else sam == 1), the other a
   multiple of 4 covering the contiguous extent, that extent (K, M or N) a multiple of 4; a and b
   16-byte aligned; c fp32 [M][ldc]; bias fp32 [N] or NULL.  colsum != NULL also writes
   colsum[n] (+)= sum_k B(k,n) (a weight gradient's db beside its dW, one pass).  Deep, narrow
   shapes split K over sae_gemm_f32_workspace_bytes(M, N, K) bytes of workspace (0: none
   needed) with a fixed-order reduction: deterministic, no atomics.
     forward  y = x W:      a = x, sam = I, sak = 1;   b = W, sbk = J, sbn = 1
     input    dx = dy W^T:  a = dy, sam = J, sak = 1;  b = W, sbk = 1, sbn = J
     weight   dW = x^T dy:  a = x, sam = 1, sak = I;   b = dy, sbk = J, sbn = 1, colsum = db */
size_t sae_gemm_f32_workspace_bytes(int32_t M, int32_t N, int32_t K);
int sae_gemm_f32(void* stream, int32_t M, int32_t N, int32_t K, const float* a, int64_t sam,
                 int64_t sak, const float* b, int64_t sbk, int64_t sbn, const float* bias, float* c,
                 int64_t ldc, float* colsum, int32_t accumulate, void* workspace);
/* fp32 Dense kernel w [K][N] -> bf16 w16 [K][N] and/or its transpose wt16 [N][K] (either may
   be NULL): the compute-dtype casts of Flax Dense (kernel cast to dtype). */
int sae_weight_cast(void* stream, int32_t K, int32_t N, const float* w, void* w16, void* wt16);
/* Many casts in one launch (every Dense kernel of a model once per step): item i casts
   w [K][N] (contiguous fp32) into columns col0 .. col0+N-1 of w16 [K][ld16] and rows
   col0 .. col0+N-1 of wt16 [*][ldT] (either may be NULL) -- e.g. the queries / keys / values
   kernels into one stacked [C][3HD] projection and its transpose. */
typedef struct sae_weight_cast_item {
  const float* w;
  void* w16;
  void* wt16;
  int32_t K, N, ld16, ldT, col0;
} sae_weight_cast_item;
int sae_weight_cast_multi(void* stream, int32_t n, const sae_weight_cast_item* items);

/* Patch embedding (models/layers/stems/patch_embed.py:15-26: einops
   'b (h ph) (w pw) c -> b (h w) (ph pw c)' then Dense) as one GEMM whose A operand is gathered
   from the images while it is staged (no patchified copy):
     out[n][p][e] = sum_k image[n][py*ph + ky][px*pw + kx][c] * wt[e][k] (+ bias[e])
   with p = py * (width / pw) + px, k = (ky * pw + kx) * channels + c.  images bf16 or fp32
   (rounded to bf16, train.py:81) in layout SAE_LAYOUT_NHWC [batch][height][width][channels]
   (the model call) or SAE_LAYOUT_HWCN [height][width][channels][batch] (the train-step feed,
   train.py:80); wt bf16 [embed][K] (the transposed bf16 kernel, sae_weight_cast), bias fp32
   [embed] or NULL, out bf16 [batch][L][embed] (L = patches per image).  Requirements:
   height % ph == width % pw == 0, K = ph*pw*channels a multiple of 64, pw*channels and embed
   multiples of 8, HWCN batch a multiple of 8, image elements < 2^31, 16-byte aligned pointers. */
#define SAE_LAYOUT_NHWC 0
#define SAE_LAYOUT_HWCN 1
typedef struct sae_patch_desc {
  int32_t batch, height, width, channels;
  int32_t patch_h, patch_w, embed;
  int32_t layout;   /* SAE_LAYOUT_* */
  int32_t dtype;    /* SAE_DTYPE_BF16 / SAE_DTYPE_F32: the images' element type */
} sae_patch_desc;
int sae_patch_embed_fwd(void* stream, const sae_patch_desc* desc, const void* images,
                        const void* wt, const float* bias, void* out);
/* Weight / bias gradients of the patch embedding: dw fp32 [K][embed] (+)= sum over tokens of
   patch[m][k] * dout[m][e], db fp32 [embed] (may be NULL); dout bf16 [batch][L][embed];
   deterministic split-token reduction through the workspace. */
size_t sae_patch_embed_bwd_workspace_bytes(const sae_patch_desc* desc);
int sae_patch_embed_bwd(void* stream, const sae_patch_desc* desc, const void* images,
                        const void* dout, float* dw, float* db, int32_t accumulate, void* workspace);
/* The patch matrix of HWCN images as bf16 rows: patches[n * L + p][k], k = (ky * Pw + kx) * C + c
   (the einops order of patch_embed.py:21), L = (H / Ph) * (W / Pw), K = Ph * Pw * C; fp32 images
   are rounded to bf16 (the same operand bits as sae_patch_embed_fwd's loaders).  The train step
   writes it once and runs the embedding as sae_gemm_nt(patches, W^T) and its weight gradient as
   sae_gemm_dw(patches, dY): the LDS-DMA GEMM kernels instead of the per-chunk eight-image scatter of
   the fused HWCN loaders.  desc as sae_patch_embed_fwd, layout SAE_LAYOUT_HWCN. */
int sae_patch_gather(void* stream, const sae_patch_desc* desc, const void* images, void* patches);

/* Residual add + LayerNorm of the encoder blocks around the path (models/vit.py:19-31,57;
   Flax nn.LayerNorm: fp32 statistics, eps, output in the compute dtype):
     xout = x + delta (fp32; when delta != NULL), y = LN(xout) * gamma + beta in bf16,
     mean / rstd fp32 [M] saved for the backward.  x, xout fp32 [M][C]; delta, y bf16 [M][C];
     C a multiple of 4, <= 1024. */
int sae_layernorm_fwd(void* stream, int32_t M, int32_t C, const float* x, const void* delta,
                      float* xout, const float* gamma, const float* beta, void* y, float* mean,
                      float* rstd, float eps);
/* CaiT form (layerscale.py:21-23, stochastic_depth.py:19-28 folded into the residual add):
     xout = x + delta * bf16(layerscale[c]) * rowscale[row / rows_per_sample]   (rowscale may be NULL)
   layerscale fp32 [C] (16-byte aligned; the parameter as stored -- the kernels round it to bf16,
   the compute-dtype cast of layerscale.py:22), rowscale fp32 [M / rows_per_sample]. */
int sae_layernorm_fwd_scaled(void* stream, int32_t M, int32_t C, const float* x, const void* delta,
                             float* xout, const float* gamma, const float* beta, void* y,
                             float* mean, float* rstd, float eps, const float* layerscale,
                             const float* rowscale, int32_t rows_per_sample);
size_t sae_layernorm_bwd_workspace_bytes(int32_t M, int32_t C);
/* dx = dxin + dLN/dx(dy) (fp32; dxin may be NULL), ddelta = bf16(dx) (may be NULL),
   dgamma / dbeta fp32 [C] overwritten (fixed-order reduction, deterministic). */
int sae_layernorm_bwd(void* stream, int32_t M, int32_t C, const float* x, const float* mean,
                      const float* rstd, const float* gamma, const void* dy, const float* dxin,
                      float* dx, void* ddelta, float* dgamma, float* dbeta, void* workspace);
/* Backward of the scaled form: ddelta = bf16(dx * layerscale * rowscale), dlayerscale[c] =
   sum over rows of dx * delta * rowscale (fixed order, with dgamma / dbeta); delta is the bf16
   addend of the forward. */
int sae_layernorm_bwd_scaled(void* stream, int32_t M, int32_t C, const float* x, const float* mean,
                             const float* rstd, const float* gamma, const void* dy, const float* dxin,
                             float* dx, void* ddelta, float* dgamma, float* dbeta, void* workspace,
                             const void* delta, const float* layerscale, const float* rowscale,
                             int32_t rows_per_sample, float* dlayerscale);

/* The plain add + LayerNorm pair with the hidden dropout on the addend (the attention-output and
   FF-output dropouts of vit.py:22-24,29-31 riding in the residual add; the mask above over [M][C]):
     forward   xout = x + delta * keep / pk   (delta required), then the LayerNorm as above
     backward  ddelta = bf16(dx * keep / pk);  dx, dgamma, dbeta as above */
int sae_layernorm_fwd_dropout(void* stream, int32_t M, int32_t C, const float* x, const void* delta,
                              float* xout, const float* gamma, const float* beta, void* y,
                              float* mean, float* rstd, float eps, float rate, const uint64_t* rng,
                              uint32_t stream_id, int64_t row0, int64_t row_step);
int sae_layernorm_bwd_dropout(void* stream, int32_t M, int32_t C, const float* x, const float* mean,
                              const float* rstd, const float* gamma, const void* dy,
                              const float* dxin, float* dx, void* ddelta, float* dgamma, float* dbeta,
                              void* workspace, float rate, const uint64_t* rng, uint32_t stream_id,
                              int64_t row0, int64_t row_step);

/* The CvT convolutional projection in front of its 1x1 convolution (cvt_attention.py:12-40):
   depthwise 3x3 convolution (stride 1 or 2, Flax SAME padding: Ho = ceil(H / stride), total padding
   max((Ho - 1) stride + 3 - H, 0) with the smaller half in front) followed by BatchNorm.
     t[b,p,q,c] = sum_{i,j} xpad[b, p stride + i, q stride + j, c] w[i,j,c]   (fp32 accumulation, i outer,
                  j inner, rounded to the compute dtype)
     training:   mu, var = biased statistics of t over N = B Ho Wo positions (fp64 sums, no
                 cancellation for a large mean), rstd = rsqrt(var + eps),
                 y = ((t - mu) rstd) gamma + beta, and the Flax running averages
                 run_mean = momentum run_mean + (1 - momentum) mu, run_var likewise with var
                 (updated on the device, stream-ordered: a captured graph advances them per replay)
     evaluation: the same formula with run_mean / run_var in one kernel; t, mean, rstd and workspace
                 may be NULL and the running buffers are not written.
   x [B][H][W][C], t and y [B][Ho][Wo][C] contiguous in the compute dtype (bf16 or fp32); w fp32
   [3][3][C] (the Flax kernel [3, 3, 1, C]; rounded to the compute dtype as it is loaded); gamma,
   beta, run_mean, run_var, mean, rstd fp32 [C].  channels must be a multiple of 8 (bf16) or 4
   (fp32); every pointer 16-byte aligned.  Every reduction has a fixed order (no atomics): two calls
   on the same inputs agree bit for bit. */
typedef struct sae_dwconv_desc {
  int32_t batch, height, width, channels;
  int32_t stride;    /* 1 or 2 */
  int32_t dtype;     /* SAE_DTYPE_* */
  int32_t training;  /* 0: evaluation (running statistics), else batch statistics */
  float momentum;    /* of the running averages (Flax convention) */
  float eps;
} sae_dwconv_desc;
/* Bytes sae_dwconv_bn_fwd / _bwd need at `workspace` for either compute dtype (0: unsupported shape):
   the per-workgroup partial rows of the reductions and, for the backward, dt (B Ho Wo C elements). */
size_t sae_dwconv_bn_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride);
int sae_dwconv_bn_fwd(void* stream, const sae_dwconv_desc* desc, const void* x, const float* w,
                      const float* gamma, const float* beta, float* run_mean, float* run_var, void* t,
                      void* y, float* mean, float* rstd, void* workspace);
/* Backward of the training form, from the t, mean, rstd the forward saved and g = dy:
     dbeta = sum g, dgamma = sum g xhat, dt = gamma rstd (g - dbeta / N - xhat dgamma / N),
     dx[b,h,w,c] = sum over taps (i,j) and outputs (p,q) with p stride + i = h + pad_top,
                   q stride + j = w + pad_left of w[i,j,c] dt[b,p,q,c]   (gather; compute dtype),
     dw[i,j,c] = sum_{b,p,q} xpad[b, p stride + i, q stride + j, c] dt[b,p,q,c]   (fp32 [3][3][C]).
   dw, dgamma, dbeta are overwritten.  desc->training == 0 is SAE_EUNSUPPORTED. */
int sae_dwconv_bn_bwd(void* stream, const sae_dwconv_desc* desc, const void* x, const float* w,
                      const float* gamma, const void* t, const float* mean, const float* rstd,
                      const void* dy, void* dx, float* dw, float* dgamma, float* dbeta, void* workspace);

/* ---- BatchNorm over token rows + tanh-GELU (CeiT LeFF, models/layers/feedforwards/leff.py:39-59) ----
   x [B][L + x_lead][C] in the compute dtype; x_lead (0 or 1) leading rows per sample (the class
   token) are skipped and N = B L rows take part.  y [B][L + y_lead][C]; with y_lead = 1 row 0 of
   every sample of y is a copy of the row of C elements at lead + b * lead_pitch (elements).
     training:   mu, var = biased batch statistics per channel (fp64 sums), r = rsqrt(var + eps),
                 z = T(((x - mu) r) gamma + beta), y = T(gelu(z)) (tanh form); mean = mu and rstd = r are
                 saved; run_mean = m run_mean + (1 - m) mu, run_var likewise, on the device in stream order
     evaluation: the same formula with run_mean / run_var; buffers untouched, mean / rstd / workspace unused
   gamma, beta, run_mean, run_var, mean, rstd fp32 [C].  channels must be a multiple of 8 (bf16) or 4
   (fp32), lead_pitch a multiple of the same, every pointer 16-byte aligned and B (L + 1) C <= 2^31 - 1;
   anything else is SAE_EUNSUPPORTED.  Fixed-order reductions (no atomics): two calls on the same inputs
   agree bit for bit.  No host synchronisation. */
typedef struct sae_bnrows_desc {
  int32_t batch, tokens, channels;
  int32_t x_lead, y_lead; /* 0 or 1 */
  int32_t dtype;          /* SAE_DTYPE_* */
  int32_t training;       /* 0: evaluation (running statistics), else batch statistics */
  float momentum;         /* of the running averages (Flax convention) */
  float eps;
} sae_bnrows_desc;
/* Bytes sae_bn_gelu_fwd / _bwd need at `workspace` for either compute dtype (0: unsupported shape). */
size_t sae_bn_gelu_workspace_bytes(int32_t B, int32_t L, int32_t C);
int sae_bn_gelu_fwd(void* stream, const sae_bnrows_desc* desc, const void* x, const float* gamma,
                    const float* beta, float* run_mean, float* run_var, const void* lead, int64_t lead_pitch,
                    void* y, float* mean, float* rstd, void* workspace);
/* Backward of the training form from x, the saved mean / rstd and g = dy (y's layout): z is recomputed
   with the forward's rounding, dz = g gelu'(z), dbeta = sum dz, dgamma = sum dz xhat,
   dx = T(gamma r (dz - dbeta / N - xhat dgamma / N)) in x's layout with the skipped lead rows written
   as zeros.  The gradient of `lead` is row 0 of every sample of dy.  dgamma, dbeta are overwritten.
   desc->training == 0 is SAE_EUNSUPPORTED. */
int sae_bn_gelu_bwd(void* stream, const sae_bnrows_desc* desc, const void* x, const float* gamma,
                    const float* beta, const float* mean, const float* rstd, const void* dy, void* dx,
                    float* dgamma, float* dbeta, void* workspace);

/* The CvT convolutional token embedding (models/cvt.py:19-35): a dense kernel x kernel convolution
   with stride < kernel and Flax SAME padding (Ho = ceil(H / stride), total padding
   max((Ho - 1) stride + kernel - H, 0), the smaller half in front), as a window matrix written once
   and the GEMMs above on it (forward P W on sae_gemm_nt / sae_gemm_f32, weight gradient P^T dY on
   sae_gemm_dw / sae_gemm_f32, input gradient the scatter of dY W^T).
     M = batch Ho Wo rows, K = kernel^2 channels columns, Kp = K rounded up to a multiple of 8
     (sae_conv_window_cols); column (ky kernel + kx) channels + c, the Flax kernel [kh, kw, in, out]
     viewed as [K, out].
   sae_conv_window_gather:  P[m][col] = x[b][oy stride - pad_top + ky][ox stride - pad_left + kx][c],
     zero for taps outside the image and for the columns K .. Kp.  x [B][H][W][channels] contiguous
     in in_dtype, P [M][Kp] contiguous in dtype (the compute dtype): bf16 or fp32 x for a bf16 P
     (fp32 values are rounded to nearest even as they are staged), fp32 x for an fp32 P.
   sae_conv_window_scatter: dX[b][iy][ix][c] = the sum of dP[m(b, oy, ox)][(ky kernel + kx) channels + c]
     over the windows with oy stride + ky = iy + pad_top, 0 <= oy < Ho (the same in x), in fp32,
     ky ascending then kx ascending; dP [M][Kp] and dX [B][H][W][channels] in dtype.  A gather over
     at most ceil(kernel / stride)^2 windows per pixel: no atomics, two calls agree bit for bit.
   16-byte chunks where channels % 8 == 0 (bf16 P / dP) or % 4 == 0 (fp32), element accesses
   otherwise; P, dP and (on the chunk path) x, dX must be 16-byte aligned.  Refused before any
   launch: kernel outside 1..7, stride < 1, an extent < 1, an unknown dtype or a bf16 x with an fp32
   P, NULL pointers, and extents whose element offsets (B H W channels, M Kp) exceed 2^31 - 1.
   No workspace; graph-capturable. */
typedef struct sae_convtok_desc {
  int32_t batch, height, width, channels;
  int32_t kernel;    /* 1..7 */
  int32_t stride;    /* >= 1 */
  int32_t in_dtype;  /* SAE_DTYPE_* of x (gather only) */
  int32_t dtype;     /* SAE_DTYPE_* of P, dP and dX: the compute dtype */
} sae_convtok_desc;
/* Kp of a descriptor's window matrix, 0 for channels < 1 or kernel outside 1..7. */
int32_t sae_conv_window_cols(int32_t channels, int32_t kernel);
int sae_conv_window_gather(void* stream, const sae_convtok_desc* desc, const void* x, void* P);
int sae_conv_window_scatter(void* stream, const sae_convtok_desc* desc, const void* dP, void* dX);

/* Optimizer update of the data-parallel training step (train.py:25-27,229-233: optax.adamw,
   survey D9 descent), every parameter in ONE launch.  The parameters are cut into chunks of
   SAE_ADAMW_CHUNK elements; sae_adamw_plan (host only, no GPU call) fills that chunk table for
   n_items fp32 tensors (item i: parameter p[i], gradient g[i], moments m[i], v[i], n[i] elements,
   contiguous) into `chunks` (capacity max_chunks) and returns the count in *n_chunks.  The caller
   copies the table to device memory once; sae_adamw_step then increments the device-resident
   step counter *step (int32) and applies, with t = the new *step (torch.optim.AdamW order):
     p *= 1 - lr*wd;  m = m + (1-b1)(g - m);  v = b2 v + (1-b2) g^2;
     p -= lr/(1 - b1^t) * m / (sqrt(v)/sqrt(1 - b2^t) + eps)
   Both launches are stream-ordered, so a captured graph replays with the right t. */
#define SAE_ADAMW_CHUNK 2048
typedef struct sae_adamw_chunk {
  float* p;
  const float* g;
  float* m;
  float* v;
  int32_t n;     /* elements of this chunk, <= SAE_ADAMW_CHUNK */
  int32_t vec;   /* set by the plan: 16-byte aligned full chunk (vector path) */
} sae_adamw_chunk;
int sae_adamw_plan(int32_t n_items, float* const* p, const float* const* g, float* const* m,
                   float* const* v, const int64_t* n, sae_adamw_chunk* chunks, int64_t max_chunks,
                   int64_t* n_chunks);
int sae_adamw_step(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int32_t* step,
                   float lr, float beta1, float beta2, float eps, float weight_decay);

/* The same update with the bf16 compute copies of the Dense kernels written by the optimizer pass
   (the per-forward fp32 -> bf16 casts of Flax Dense, sae_weight_cast_multi, move into the
   update): item i is a Dense kernel p[i] fp32 [K[i]][N[i]] (contiguous, gradient and moments laid
   out alike) whose updated values are also stored as bf16 into columns col0[i] .. col0[i] + N[i]
   of w16[i] [K][ld16[i]] and rows col0[i] .. of wt16[i] [*][ldT[i]] (either may be NULL).
   sae_adamw_cast_plan (host only) cuts the items into 64 x 64 tiles (K, N, col0, ld16, ldT
   multiples of 4; p / g / m / v 16-byte, w16 / wt16 8-byte aligned: SAE_EUNSUPPORTED otherwise);
   sae_adamw_step_cast runs the chunk table (the other parameters) and the tile table in ONE launch
   after the step-counter tick.  The parameter values are bit-identical to sae_adamw_step's. */
typedef struct sae_adamw_cast_tile {
  float* p;
  const float* g;
  float* m;
  float* v;
  void* w16;
  void* wt16;
  int32_t K, N, ld16, ldT, col0, k0, n0, pad;
} sae_adamw_cast_tile;
int sae_adamw_cast_plan(int32_t n_items, float* const* p, const float* const* g, float* const* m,
                        float* const* v, const int32_t* K, const int32_t* N, void* const* w16,
                        const int32_t* ld16, void* const* wt16, const int32_t* ldT, const int32_t* col0,
                        sae_adamw_cast_tile* tiles, int64_t max_tiles, int64_t* n_tiles);
int sae_adamw_step_cast(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int64_t n_tiles,
                        const sae_adamw_cast_tile* tiles, int32_t* step, float lr, float beta1, float beta2,
                        float eps, float weight_decay);

/* The reference's optimizer chain around that update (train.py:22-27,214-220: optax.chain of
   clip_by_global_norm(max_norm), scale_by_adam, additive_weight_decay, scale_by_schedule of
   warmup_cosine_decay_schedule).  The two values that change every step live in device memory,
   hyper = {lr_t, clip_scale, grad_norm, unused} (4 floats), so a captured graph replays with
   this step's rate and this step's clip.

   sae_adamw_prepare takes the place of the step-counter tick.  It
     1. computes the global norm of the contiguous fp32 gradient buffer g[0..n): one workgroup
        per SAE_ADAMW_NORM_SPAN elements writes one fp64 partial sum of squares to `workspace`
        (sae_adamw_prepare_workspace_bytes(n) bytes, 8-byte aligned; squares and sums in fp64, no
        atomics: two calls on the same data give the same bits), 16-byte loads when g is 16-byte
        aligned, scalar loads otherwise;
     2. in one workgroup adds the partials in a fixed order (SAE_ADAMW_PREPARE_PASS per pass) and
        writes grad_norm = sqrt(sum) and clip_scale = grad_norm < max_norm ? 1 : max_norm / grad_norm
        (a zero norm gives 1; a NaN norm gives NaN, an infinite one 0: nothing is skipped
        silently; max_norm = +inf only monitors the norm);
     3. writes lr_t = the schedule at count = *step, the number of updates already applied (as
        optax counts), then increments *step.
   With n == 0 and g == workspace == NULL step 1 is left out (grad_norm 0, clip_scale 1).
   Schedules: SAE_LR_CONSTANT (lr_t = peak) and SAE_LR_WARMUP_COSINE, as optax composes it:
     count < warmup_steps:  init + (peak - init) count / warmup_steps
     otherwise, c = min(count - warmup_steps, D), D = decay_steps - warmup_steps, a = end / peak:
                            peak ((1 - a) (1 + cos(pi c / D)) / 2 + a)
   SAE_EINVAL: NULL schedule / step / hyper, n < 1 or a NULL g / workspace (unless all three are
   0 / NULL), max_norm <= 0 or NaN, an unknown kind, peak <= 0 or not finite, warmup_steps < 0,
   decay_steps <= warmup_steps, init / end negative or not finite.

   sae_adamw_step_dev is sae_adamw_step (n_tiles == 0) / sae_adamw_step_cast without the tick, with
   lr = hyper[0] and every gradient multiplied by hyper[1] (rounded to fp32) before the same
   arithmetic; with clip_scale 1 its results are bit-identical to theirs.  Call it after
   sae_adamw_prepare on the same stream. */
#define SAE_ADAMW_NORM_SPAN 16384
#define SAE_ADAMW_PREPARE_PASS 256
#define SAE_LR_CONSTANT 0
#define SAE_LR_WARMUP_COSINE 1
typedef struct sae_lr_schedule {
  int32_t kind;          /* SAE_LR_* */
  float init, peak, end; /* SAE_LR_CONSTANT reads peak only */
  int32_t warmup_steps, decay_steps;
} sae_lr_schedule;
size_t sae_adamw_prepare_workspace_bytes(int64_t n);
int sae_adamw_prepare(void* stream, int64_t n, const float* g, float max_norm, const sae_lr_schedule* schedule,
                      int32_t* step, void* workspace, float* hyper);
int sae_adamw_step_dev(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int64_t n_tiles,
                       const sae_adamw_cast_tile* tiles, const int32_t* step, const float* hyper, float beta1,
                       float beta2, float eps, float weight_decay);

/* Encoder input of ViT / DeiT (models/vit.py:82-85 class-token concatenate, vit.py:46 +
   position_embed.py:48 AddAbsPosEmbed), tokens bf16 [B][L][E] from the patch embedding, cls fp32
   [E], pos fp32 [L+1][E]:  x fp32 [B][L+1][E] = concat(cls, float(tokens)) + pos.  Backward:
   dtokens bf16 [B][L][E] = bf16(dx[:, 1:]), dpos [L+1][E] = sum_b dx[b], dcls [E] = dpos[0] (may be
   NULL); batch sums in a fixed order.  E % 4 == 0, E <= 4096; x / dx / cls / pos / dpos / dcls
   16-byte and tokens / dtokens 8-byte aligned. */
int sae_tokens_fwd(void* stream, int32_t B, int32_t L, int32_t E, const void* tokens, const float* cls,
                   const float* pos, float* x);
int sae_tokens_bwd(void* stream, int32_t B, int32_t L, int32_t E, const float* dx, void* dtokens, float* dcls,
                   float* dpos);

/* The same with the encoder-input dropout of vit.py:47 (the hidden-state mask above over rows
   b * (L + 1) + n, columns E):  x = (concat(cls, tokens) + pos) * keep / pk;  backward with
   g = dx * keep / pk: dtokens = bf16(g[:, 1:]), dpos = sum_b g[b] in the same fixed order,
   dcls = dpos[0]. */
int sae_tokens_fwd_dropout(void* stream, int32_t B, int32_t L, int32_t E, const void* tokens,
                           const float* cls, const float* pos, float* x, float rate,
                           const uint64_t* rng, uint32_t stream_id);
int sae_tokens_bwd_dropout(void* stream, int32_t B, int32_t L, int32_t E, const float* dx, void* dtokens,
                           float* dcls, float* dpos, float rate, const uint64_t* rng,
                           uint32_t stream_id);

/* Label-smoothed softmax cross entropy of the training step (replaces train.py:77-90:
   optax.smooth_labels(one_hot(labels), alpha) + jnp.mean(optax.softmax_cross_entropy)):
     loss = mean_r [ lse_r - (1 - alpha) x[r, labels[r]] - (alpha / classes) sum_c x[r, c] ]
   logits x [rows][classes] (row stride ld elements, dtype SAE_DTYPE_BF16 or SAE_DTYPE_F32),
   labels int64 [rows] (a label outside [0, classes) contributes no target term).  fwd writes
   lse [rows] (fp32, for the backward), row_loss [rows] (fp32) and *loss (fp32, device memory);
   the row losses are summed in a fixed order (deterministic).  bwd writes dlogits [rows][classes] (row stride ldd, the logits'
   dtype) = (*grad_loss / rows) (softmax(x_r) - (1 - alpha) onehot - alpha / classes).
   rows <= SAE_CE_MAX_ROWS. */
#define SAE_CE_MAX_ROWS 16384
int sae_smoothed_ce_fwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                        int32_t dtype, const int64_t* labels, float alpha, float* lse, float* row_loss,
                        float* loss);
int sae_smoothed_ce_bwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                        int32_t dtype, const int64_t* labels, float alpha, const float* lse,
                        const float* grad_loss, void* dlogits, int64_t ldd);

/* The same loss against mixup / cutmix targets (train.py:83-90 with the default augmentation:
   rho onehot(labels) + (1 - rho) onehot(mix_labels), then optax.smooth_labels), with the top-k
   ranks of utils.topk_correct (train.py:98-99) from the same pass:
     row_loss_r = lse_r - (1 - alpha) (rho_r x[r, labels[r]] + (1 - rho_r) x[r, mix_labels[r]])
                  - (alpha / classes) sum_c x[r, c]
   mix_labels (int64 [rows]) and ratio (fp32 [rows], rho) are both NULL (one label per row) or both
   set.  sae_smoothed_ce_fwd / _bwd is this pair with mix_labels, ratio, rank and top NULL (one host
   path, one kernel family); ratio == 1 with finite logits gives the same bits of lse, row_loss,
   *loss and dlogits as NULL does.  rank (int32 [rows]) and top (fp32 [2], device
   memory) are both NULL (no metrics) or both set: rank[r] = the number of classes a stable
   ascending argsort of row r places above labels[r] -- class c ranks above label y iff x[c] > x[y],
   or x[c] is NaN and x[y] is not, or they compare equal (-0 == +0; both NaN) and c > y; a label
   outside [0, classes) gets rank = classes -- and top[0], top[1] = the fractions of rows with
   rank < 1 and rank < 5.  bwd writes dlogits = (*grad_loss / rows) (softmax(x_r)
   - (1 - alpha) (rho [c == labels[r]] + (1 - rho) [c == mix_labels[r]]) - alpha / classes). */
int sae_mixed_ce_fwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld, int32_t dtype,
                     const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha, float* lse,
                     float* row_loss, int32_t* rank, float* loss, float* top);
int sae_mixed_ce_bwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld, int32_t dtype,
                     const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha,
                     const float* lse, const float* grad_loss, void* dlogits, int64_t ldd);

/* Evaluation totals: adds one batch's row_loss / rank (as sae_mixed_ce_fwd wrote them) into the
   SAE_CE_ACCUM_BYTES device accumulator acc = {double loss_sum; int64_t top1, top5, samples} (8-byte
   aligned; the caller zeroes it).  The losses are added in double, in row order.  Stream-ordered, no
   atomics: replays of a captured graph keep accumulating. */
#define SAE_CE_ACCUM_BYTES 32
int sae_ce_accumulate(void* stream, int32_t rows, const float* row_loss, const int32_t* rank, void* acc);

/* Diagnostic: occupy `workgroups` workgroups of `threads` threads, each holding `lds_bytes` of LDS,
   for `usec` microseconds (a timed s_sleep loop, no memory traffic), on `stream`.  Used by
   bench.py --emulate-rccl to stand in, on one GPU, for the RCCL all-reduce kernels that share the
   CUs with the backward on an 8-GPU node (one workgroup per ring channel, busy for the bucket's
   ring time).  threads in [64, 1024], lds_bytes <= 160 KiB. */
int sae_occupy_cus(void* stream, int32_t workgroups, int32_t threads, int32_t lds_bytes, float usec);

/* Stream-ordered flags for collectives gated outside a HIP graph (train.py, the data-parallel step):
   sae_flag_bump adds 1 to flags[index] (a one-thread kernel; system-scope atomic after the stream's
   earlier kernels, whose writes the kernel boundary has made visible), so a graph can mark points of
   its kernel chain without forking a branch; sae_stream_wait_flag makes `stream` wait until
   *flag >= value (hipStreamWaitValue32, greater-or-equal) before its later work starts. */
int sae_flag_bump(void* stream, uint32_t* flags, int32_t index);
int sae_stream_wait_flag(void* stream, const uint32_t* flag, uint32_t value);

/* Thread-local message describing the last failure on this thread ("" if none). */
const char* sae_last_error(void);

/* ABI version (SAE_ABI_VERSION) and a build string. */
int32_t sae_abi_version(void);
const char* sae_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SAE_ATTN_H */

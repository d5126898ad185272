// misc.hip -- the rest of the C ABI: residual add + LayerNorm (ln.h), the encoder input tokens
// (tokens.h), the hidden-state dropout of row-major activations (drop_rows.h: their dropout forms
// and the standalone kernels), the cross-entropy family (label-smoothed, mixup / cutmix targets, top-k)
// and the evaluation accumulator (loss.h), AdamW (adamw.h), the CvT convolutional projection
// (depthwise 3x3 + BatchNorm, dwconv.h), the CeiT LeFF block's BatchNorm + GELU over token rows
// (bn_rows.h), the CvT convolutional token embedding's window matrix (convtok.h), the stream utilities of bench.py, and the library's error string and version.
#include "ln.h"
#include "dwconv.h"
#include "bn_rows.h"
#include "convtok.h"
#include "loss.h"
#include "tokens.h"
#include "adamw.h"
#include "host.h"

namespace sae {

// ------------------------------------------------------------------------ standalone kernels
// y = x * keep / pk on [M][C] (row strides ldx / ldy; y may alias x): the paths the fused forms do
// not take (fp32 compute dtype, shapes outside an envelope) and its own backward.  One thread per
// 4 consecutive columns (one Philox word); HBM-bound.  vec (set by the host: C and both strides
// multiples of 4, both pointers aligned to 4 elements): one vector load and store per thread.
struct DropRowsArgs {
  const void* x;
  void* y;
  unsigned char* keep;   // the mask kernel's output [M][C]
  long long ldx, ldy;
  int M, C, vec;
  DropRows d;
};

template <typename T>
__global__ __launch_bounds__(256) void dropout_rows_kernel(DropRowsArgs a) {
  const int C4 = (a.C + 3) / 4;
  const long long total = (long long)a.M * C4;
  const DropKey dk = drop_key(a.d.rng, a.d.stream_id);
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    const long long r = i / C4;
    const unsigned long long row = (unsigned long long)(a.d.row0 + r * a.d.row_step);
    const unsigned w = drop_word(drop_rows_call(dk, row, (unsigned)c4 >> 2), (unsigned)c4 & 3u);
    const f32x4 s = drop_scale4(w, a.d.thr, a.d.inv);
    const T* xp = reinterpret_cast<const T*>(a.x) + r * a.ldx + 4 * c4;
    T* yp = reinterpret_cast<T*>(a.y) + r * a.ldy + 4 * c4;
    if (a.vec) {
      typedef __attribute__((ext_vector_type(4))) T vec4;
      const vec4 v = *reinterpret_cast<const vec4*>(xp);
      *reinterpret_cast<vec4*>(yp) = vec4{(T)((float)v[0] * s[0]), (T)((float)v[1] * s[1]), (T)((float)v[2] * s[2]),
                                          (T)((float)v[3] * s[3])};
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * c4 + e < a.C) yp[e] = (T)((float)xp[e] * s[e]);
  }
}

// keep[M][C] as uint8 0 / 1: one thread per element (a test and debugging aid)
__global__ __launch_bounds__(256) void dropout_rows_mask_kernel(DropRowsArgs a) {
  const long long total = (long long)a.M * a.C;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const DropKey dk = drop_key(a.d.rng, a.d.stream_id);
  const unsigned col = (unsigned)(i % a.C);
  const long long r = i / a.C;
  a.keep[i] = drop_rows_keep(dk, a.d.thr, (unsigned long long)(a.d.row0 + r * a.d.row_step), col) ? 1 : 0;
}

}  // namespace sae

using namespace sae;

thread_local std::string sae::g_err;

namespace {

// ------------------------------------------------------------ residual add + LayerNorm
// rows per wave: with the rows software-pipelined (ln.h) fewer, longer-lived waves win -- 2048 / 1024
// -> 1024 / 512 workgroups: DeiT-S step 8.220 -> 8.174 ms same box (profiles/r05ac_ln_grid_ab.txt;
// before the pipelining, 512 backward workgroups were slower: too few rows in flight)
int ln_fwd_blocks(int M) { return std::max(1, std::min((M + 3) / 4, 1024)); }
int ln_bwd_blocks(int M) { return std::max(1, std::min((M + 3) / 4, 512)); }

int ln_check(int32_t M, int32_t C) {
  if (M < 1 || C < 4) return fail(SAE_EINVAL, "layernorm: M (%d) and C (%d) must be >= 1 / >= 4", M, C);
  if (C % 4 || C > 4 * 64 * kLnMaxV)
    return fail(SAE_EUNSUPPORTED, "layernorm: C (%d) must be a multiple of 4 and <= %d", C, 4 * 64 * kLnMaxV);
  return SAE_OK;
}

// drop != nullptr: the dropout form (lsc / rsc unused)
int ln_fwd_impl(void* stream, int32_t M, int32_t C, const float* x, const void* delta, float* xout,
                const float* gamma, const float* beta, void* y, float* mean, float* rstd, float eps,
                const float* lsc, const float* rsc, int32_t rpb, const DropRows* drop = nullptr) {
  if (int rc = ln_check(M, C)) return rc;
  if (!x || !gamma || !beta || !y || !mean || !rstd) return fail(SAE_EINVAL, "layernorm_fwd: NULL argument");
  if ((delta == nullptr) != (xout == nullptr))
    return fail(SAE_EINVAL, "layernorm_fwd: delta and xout must both be given or both be NULL");
  if (!aligned16(x) || !aligned16(xout) || !aligned16(gamma) || !aligned16(beta) || ((uintptr_t)delta & 7) ||
      ((uintptr_t)y & 7))
    return fail(SAE_EINVAL, "layernorm_fwd: x/xout/gamma/beta need 16-byte, delta/y 8-byte alignment");
  LnArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.delta = reinterpret_cast<const __bf16*>(delta);
  a.xout = xout;
  a.gamma = gamma;
  a.beta = beta;
  a.y = reinterpret_cast<__bf16*>(y);
  a.mean = mean;
  a.rstd = rstd;
  a.M = M;
  a.C = C;
  a.eps = eps;
  a.lsc = lsc;
  a.rsc = rsc;
  a.rpb = rpb > 0 ? rpb : 1;
  int lnb = ln_fwd_blocks(M);
  if (int v = dev_knob("SAE_LN_FWD_BLOCKS")) lnb = std::max(1, std::min((M + 3) / 4, v));
  void (*const fn[4])(LnArgs) = {ln_fwd_kernel<1>, ln_fwd_kernel<2>, ln_fwd_kernel<3>, ln_fwd_kernel<4>};
  void (*const fnd[4])(LnArgs) = {ln_fwd_kernel<1, true>, ln_fwd_kernel<2, true>, ln_fwd_kernel<3, true>,
                                  ln_fwd_kernel<4, true>};
  const int nv = (C / 4 + 63) / 64;   // 1 .. kLnMaxV (ln_check)
  if (drop) {
    a.drop = *drop;
    return launch("layernorm_fwd_dropout", fnd[nv - 1], (long long)lnb, dim3(256), 0, (hipStream_t)stream, a);
  }
  return launch("layernorm_fwd", fn[nv - 1], (long long)lnb, dim3(256), 0, (hipStream_t)stream, a);
}

int ln_bwd_impl(void* stream, int32_t M, int32_t C, const float* x, const float* mean, const float* rstd,
                const float* gamma, const void* dy, const float* dxin, float* dx, void* ddelta,
                float* dgamma, float* dbeta, void* workspace, const void* delta, const float* lsc,
                const float* rsc, int32_t rpb, float* dlsc, const DropRows* drop = nullptr) {
  if (int rc = ln_check(M, C)) return rc;
  if (!x || !mean || !rstd || !gamma || !dy || !dx || !dgamma || !dbeta || !workspace)
    return fail(SAE_EINVAL, "layernorm_bwd: NULL argument");
  if (!aligned16(x) || !aligned16(dxin) || !aligned16(dx) || !aligned16(gamma) || !aligned16(workspace) ||
      ((uintptr_t)dy & 7) || ((uintptr_t)ddelta & 7))
    return fail(SAE_EINVAL, "layernorm_bwd: x/dxin/dx/gamma/workspace need 16-byte, dy/ddelta 8-byte alignment");
  LnArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.mean = const_cast<float*>(mean);
  a.rstd = const_cast<float*>(rstd);
  a.gamma = gamma;
  a.dy = reinterpret_cast<const __bf16*>(dy);
  a.dxin = dxin;
  a.dx = dx;
  a.ddelta = reinterpret_cast<__bf16*>(ddelta);
  a.part = reinterpret_cast<float*>(workspace);
  a.dgamma = dgamma;
  a.dbeta = dbeta;
  a.M = M;
  a.C = C;
  a.nblk = ln_bwd_blocks(M);
  if (int v = dev_knob("SAE_LN_BWD_BLOCKS")) a.nblk = std::max(1, std::min(a.nblk, v));   // (workspace: <= default)
  a.delta = reinterpret_cast<const __bf16*>(delta);
  a.lsc = lsc;
  a.rsc = rsc;
  a.rpb = rpb > 0 ? rpb : 1;
  a.dlsc = dlsc;
  hipStream_t st = (hipStream_t)stream;
  const bool sc = lsc != nullptr;   // the scaled form: three partial rows (dgamma, dbeta, dlayerscale)
  void (*const fn[4][2])(LnArgs) = {{ln_bwd_kernel<1, 2>, ln_bwd_kernel<1, 3>}, {ln_bwd_kernel<2, 2>, ln_bwd_kernel<2, 3>},
                                    {ln_bwd_kernel<3, 2>, ln_bwd_kernel<3, 3>}, {ln_bwd_kernel<4, 2>, ln_bwd_kernel<4, 3>}};
  void (*const fnd[4])(LnArgs) = {ln_bwd_kernel<1, 2, true>, ln_bwd_kernel<2, 2, true>, ln_bwd_kernel<3, 2, true>,
                                  ln_bwd_kernel<4, 2, true>};
  const int nv = (C / 4 + 63) / 64;   // 1 .. kLnMaxV (ln_check)
  if (drop) a.drop = *drop;
  if (int rc = drop ? launch("layernorm_bwd_dropout", fnd[nv - 1], (long long)a.nblk, dim3(256), 0, st, a)
                    : launch("layernorm_bwd", fn[nv - 1][sc], (long long)a.nblk, dim3(256), 0, st, a))
    return rc;
  const long long rg = ((sc ? 3 : 2) * (C / 4) + kLnRedCols - 1) / kLnRedCols;
  return launch("layernorm_bwd_reduce", sc ? ln_bwd_reduce_kernel<3> : ln_bwd_reduce_kernel<2>, rg, dim3(256), 0, st, a);
}

// ------------------------------------------------------------------ encoder input tokens
int tokens_check(int32_t B, int32_t L, int32_t E) {
  if (B < 1 || L < 1 || E < 4 || E % 4 || E > 4096)
    return fail(SAE_EINVAL, "tokens: B %d, L %d, E %d (E a multiple of 4, <= 4096)", B, L, E);
  return 0;
}

// drop != nullptr: the dropout forms
int tokens_fwd_impl(void* stream, int32_t B, int32_t L, int32_t E, const void* tokens, const float* cls,
                    const float* pos, float* x, const DropRows* drop) {
  if (int rc = tokens_check(B, L, E)) return rc;
  if (!tokens || !cls || !pos || !x) return fail(SAE_EINVAL, "tokens_fwd: NULL argument");
  if (!aligned16(cls) || !aligned16(pos) || !aligned16(x) || ((uintptr_t)tokens & 7))
    return fail(SAE_EINVAL, "tokens_fwd: cls / pos / x need 16-byte, tokens 8-byte alignment");
  const long long total = (long long)B * (L + 1) * (E / 4);
  const long long grid = std::min<long long>((total + 255) / 256, 8192);
  if (drop)
    return launch("tokens_fwd_dropout", tokens_fwd_drop_kernel, grid, dim3(256), 0, (hipStream_t)stream,
                  reinterpret_cast<const __bf16*>(tokens), cls, pos, x, B, L, E, *drop);
  return launch("tokens_fwd", tokens_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const __bf16*>(tokens), cls, pos, x, B, L, E);
}

int tokens_bwd_impl(void* stream, int32_t B, int32_t L, int32_t E, const float* dx, void* dtokens, float* dcls,
                    float* dpos, const DropRows* drop) {
  if (int rc = tokens_check(B, L, E)) return rc;
  if (!dx || !dtokens || !dpos) return fail(SAE_EINVAL, "tokens_bwd: NULL argument");
  if (!aligned16(dx) || !aligned16(dpos) || (dcls && !aligned16(dcls)) || ((uintptr_t)dtokens & 7))
    return fail(SAE_EINVAL, "tokens_bwd: dx / dcls / dpos need 16-byte, dtokens 8-byte alignment");
  const int E4 = E / 4;
  const int G = std::max(1, std::min(B, 512 / E4));
  if (drop)
    return launch("tokens_bwd_dropout", tokens_bwd_drop_kernel, (long long)L + 1, dim3((unsigned)(G * E4)),
                  (size_t)G * E4 * 16, (hipStream_t)stream, dx, reinterpret_cast<__bf16*>(dtokens), dcls, dpos, B, L,
                  E, *drop);
  return launch("tokens_bwd", tokens_bwd_kernel, (long long)L + 1, dim3((unsigned)(G * E4)), (size_t)G * E4 * 16,
                (hipStream_t)stream, dx, reinterpret_cast<__bf16*>(dtokens), dcls, dpos, B, L, E);
}

// ------------------------------------------------------------------ training loss
// One host path for the loss family of loss.h; `what` is the entry point called, so a refusal names
// it.  mix_labels / ratio both NULL (one label per row) or both set; rank / top both NULL (no
// metrics: the RANK == false kernels) or both set.  Every refusal returns before any HIP call.
int ce_check(const char* what, int32_t rows, int32_t classes, const void* logits, int64_t ld, int32_t dtype,
             const int64_t* labels, const int64_t* mix_labels, const float* ratio) {
  if (rows < 1 || rows > SAE_CE_MAX_ROWS || classes < 1 || ld < classes)
    return fail(SAE_EINVAL, "%s: rows %d (1..%d), classes %d, ld %lld", what, rows, SAE_CE_MAX_ROWS, classes,
                (long long)ld);
  if (dtype != SAE_DTYPE_BF16 && dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "%s: bad dtype %d", what, dtype);
  if (!logits || !labels) return fail(SAE_EINVAL, "%s: NULL logits / labels", what);
  if ((mix_labels == nullptr) != (ratio == nullptr))
    return fail(SAE_EINVAL, "%s: mix_labels and ratio must both be given or both be NULL", what);
  return 0;
}

int ce_fwd_impl(const char* what, void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                int32_t dtype, const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha,
                float* lse, float* row_loss, int32_t* rank, float* loss, float* top) {
  if (int rc = ce_check(what, rows, classes, logits, ld, dtype, labels, mix_labels, ratio)) return rc;
  if ((rank == nullptr) != (top == nullptr))
    return fail(SAE_EINVAL, "%s: rank and top must both be given or both be NULL", what);
  if (!lse || !row_loss || !loss) return fail(SAE_EINVAL, "%s: NULL lse / row_loss / loss", what);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = by_dtype(dtype, [&](auto* t) {
        using T = std::remove_pointer_t<decltype(t)>;
        return launch("ce_fwd", rank ? ce_fwd_kernel<T, true> : ce_fwd_kernel<T, false>, (long long)rows, dim3(256), 0,
                      st, reinterpret_cast<const T*>(logits), (long long)ld, labels, mix_labels, ratio, classes, alpha,
                      lse, row_loss, (int*)rank);
      }))
    return rc;
  return launch("ce_mean", rank ? ce_mean_kernel<true> : ce_mean_kernel<false>, 1LL, dim3(256), 0, st,
                (const float*)row_loss, (const int*)rank, rows, loss, top);
}

int ce_bwd_impl(const char* what, void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                int32_t dtype, const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha,
                const float* lse, const float* grad_loss, void* dlogits, int64_t ldd) {
  if (int rc = ce_check(what, rows, classes, logits, ld, dtype, labels, mix_labels, ratio)) return rc;
  if (!lse || !grad_loss || !dlogits || ldd < classes)
    return fail(SAE_EINVAL, "%s: NULL lse / grad_loss / dlogits or ldd < classes", what);
  return by_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch("ce_bwd", mix_labels ? ce_bwd_kernel<T, true> : ce_bwd_kernel<T, false>, (long long)rows, dim3(256), 0,
                  (hipStream_t)stream, reinterpret_cast<const T*>(logits), (long long)ld, labels, mix_labels, ratio, rows,
                  classes, alpha, lse, grad_loss, reinterpret_cast<T*>(dlogits), (long long)ldd);
  });
}


// ------------------------------------------------- depthwise 3x3 convolution + BatchNorm (CvT)
// The launch geometry of dwconv.h for one element type (V channels per 16-byte vector).  Partial
// rows cost workspace traffic (16 bytes per channel and workgroup for the fp64 pairs, 36 for dw), so
// the grids are capped: 1024 workgroups, and for the dw pass as many as keep its partials near 4 MB.
constexpr int kDwMaxBlocks = 1024;

struct DwGrid {
  int chunks, fwd, pix, dx, dw;
};

int dw_blocks(long long work, int per_block, int cap) {
  return (int)std::max<long long>(1, std::min<long long>((work + per_block - 1) / per_block, cap));
}

DwGrid dw_geometry(const sae_dwconv_desc& d, int V, DwConvArgs& a) {
  const int s = d.stride;
  a.B = d.batch;
  a.H = d.height;
  a.W = d.width;
  a.C = d.channels;
  a.Ho = (a.H + s - 1) / s;
  a.Wo = (a.W + s - 1) / s;
  a.pt = std::max((a.Ho - 1) * s + 3 - a.H, 0) / 2;   // Flax SAME: the smaller half in front
  a.pl = std::max((a.Wo - 1) * s + 3 - a.W, 0) / 2;
  const int CV = a.C / V;
  a.CVt = std::min(CV, 256);
  a.PS = 256 / a.CVt;
  a.rpr = (a.Wo + kDwRun - 1) / kDwRun;
  a.nruns = a.B * a.Ho * a.rpr;
  a.rpr_in = (a.W + kDwRun - 1) / kDwRun;
  a.nruns_in = a.B * a.H * a.rpr_in;
  a.npix = (long long)a.B * a.Ho * a.Wo;
  a.momentum = d.momentum;
  a.eps = d.eps;
  DwGrid g;
  g.chunks = (CV + a.CVt - 1) / a.CVt;
  g.fwd = dw_blocks(a.nruns, a.PS, kDwMaxBlocks);
  g.pix = dw_blocks(a.npix, a.PS * kDwPix, kDwMaxBlocks);
  g.dx = dw_blocks(a.nruns_in, a.PS, kDwMaxBlocks);
  g.dw = dw_blocks(a.nruns, a.PS, std::max(256, std::min(kDwMaxBlocks, (4 << 20) / (36 * a.C))));
  return g;
}

// bytes of the partial rows (a multiple of 16: C % 4 == 0); the backward's dt follows them
size_t dw_partial_bytes(const sae_dwconv_desc& d, int V) {
  DwConvArgs a;
  const DwGrid g = dw_geometry(d, V, a);
  return std::max((size_t)std::max(g.fwd, g.pix) * 2 * a.C * sizeof(double), (size_t)g.dw * 9 * a.C * sizeof(float));
}

size_t dw_workspace(const sae_dwconv_desc& d, int V) {
  DwConvArgs a;
  dw_geometry(d, V, a);
  return dw_partial_bytes(d, V) + (size_t)a.npix * a.C * (V == 8 ? 2 : 4);
}

// everything but the pointers; every refusal returns before any HIP call
int dw_check(const char* what, const sae_dwconv_desc* d) {
  if (!d) return fail(SAE_EINVAL, "%s: NULL descriptor", what);
  if (d->batch < 1 || d->height < 1 || d->width < 1 || d->channels < 1)
    return fail(SAE_EINVAL, "%s: batch %d, height %d, width %d, channels %d must be >= 1", what, d->batch, d->height,
                d->width, d->channels);
  if (d->dtype != SAE_DTYPE_BF16 && d->dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "%s: bad dtype %d", what, d->dtype);
  if (d->stride != 1 && d->stride != 2) return fail(SAE_EUNSUPPORTED, "%s: stride %d (1 or 2)", what, d->stride);
  const int V = d->dtype == SAE_DTYPE_BF16 ? 8 : 4;
  if (d->channels % V)
    return fail(SAE_EUNSUPPORTED, "%s: channels %d must be a multiple of %d in %s", what, d->channels, V,
                d->dtype == SAE_DTYPE_BF16 ? "bf16" : "fp32");
  if ((long long)d->batch * d->height * d->width > (1LL << 30))
    return fail(SAE_EUNSUPPORTED, "%s: batch * height * width > 2^30", what);
  return SAE_OK;
}

template <typename T>
int dw_fwd_launch(hipStream_t st, const sae_dwconv_desc& d, DwConvArgs& a) {
  const DwGrid g = dw_geometry(d, DwVec<T>::N, a);
  const dim3 gf((unsigned)g.fwd, (unsigned)g.chunks), gp((unsigned)g.pix, (unsigned)g.chunks);
  if (!d.training)
    return launch("dwconv_bn_eval", d.stride == 1 ? dwconv_fwd_kernel<T, 1, false> : dwconv_fwd_kernel<T, 2, false>, gf,
                  dim3(256), 0, st, a);
  a.nparts = g.fwd;
  if (int rc = launch("dwconv_fwd", d.stride == 1 ? dwconv_fwd_kernel<T, 1, true> : dwconv_fwd_kernel<T, 2, true>, gf,
                      dim3(256), 0, st, a))
    return rc;
  if (int rc = launch("dwconv_stats", dwconv_reduce_kernel<double, true>, (long long)(a.C + kDwRedC - 1) / kDwRedC, dim3(256), 0, st,
                      a, a.C, (float*)nullptr, (float*)nullptr, 0))
    return rc;
  return launch("dwconv_norm", dwconv_norm_kernel<T>, gp, dim3(256), 0, st, a);
}

template <typename T>
int dw_bwd_launch(hipStream_t st, const sae_dwconv_desc& d, DwConvArgs& a) {
  const DwGrid g = dw_geometry(d, DwVec<T>::N, a);
  const dim3 gp((unsigned)g.pix, (unsigned)g.chunks), gx((unsigned)g.dx, (unsigned)g.chunks),
      gw((unsigned)g.dw, (unsigned)g.chunks);
  a.nparts = g.pix;
  if (int rc = launch("dwconv_bwd_sums", dwconv_bwd_sums_kernel<T>, gp, dim3(256), 0, st, a)) return rc;
  if (int rc = launch("dwconv_bwd_sums_reduce", dwconv_reduce_kernel<double, false>, (long long)(2 * a.C + kDwRedC - 1) / kDwRedC,
                      dim3(256), 0, st, a, 2 * a.C, a.dbeta, a.dgamma, a.C))
    return rc;
  a.nparts = g.dw;
  a.dt = reinterpret_cast<char*>(a.part) + dw_partial_bytes(d, DwVec<T>::N);
  if (int rc = launch("dwconv_dw", d.stride == 1 ? dwconv_dw_kernel<T, 1> : dwconv_dw_kernel<T, 2>, gw, dim3(256), 0, st, a))
    return rc;
  if (int rc = launch("dwconv_dw_reduce", dwconv_reduce_kernel<float, false>, (long long)(9 * a.C + kDwRedC - 1) / kDwRedC,
                      dim3(256), 0, st, a, 9 * a.C, a.dw, (float*)nullptr, 9 * a.C))
    return rc;
  void (*const fx[3])(DwConvArgs) = {dwconv_dx_kernel<T, 1, 1>, dwconv_dx_kernel<T, 2, 0>, dwconv_dx_kernel<T, 2, 1>};
  return launch("dwconv_dx", fx[d.stride == 1 ? 0 : 1 + a.pl], gx, dim3(256), 0, st, a);
}


// ------------------------------------------------- BatchNorm + GELU over token rows (CeiT LeFF)
// The launch geometry of bn_rows.h for one element type.  A workgroup's 256 threads are PS row slots
// x CVt channel vectors; the C / V channel vectors are cut into `chunks` equal runs of CVt >= 8
// vectors (128-byte runs of a row) so that PS CVt comes closest to 256 live threads (C = 768 in
// bf16: 3 chunks of 32 vectors x 8 slots, not 96 vectors x 2 slots with 64 threads idle).  The
// statistics grids are capped like the dw pass of the depthwise convolution: their fp64 partial
// rows (16 bytes per channel and workgroup) stay near 4 MB.
struct BnGrid {
  int chunks, sums, apply, dx;
};

BnGrid bn_geometry(const sae_bnrows_desc& d, int V, DwConvArgs& a, BnRows& r) {
  a.C = d.channels;
  const int CV = a.C / V;
  int best = 0, chunks = 1;
  for (int n = (CV + 255) / 256; n <= CV; ++n) {
    const int cvt = (CV + n - 1) / n;
    if (cvt < 8 && n > (CV + 255) / 256) break;
    const int live = 256 / cvt * CV;   // live threads of the n workgroups of one row-slot set
    if (live * chunks > best * n) {    // live / n > best / chunks
      best = live;
      chunks = n;
    }
  }
  a.CVt = (CV + chunks - 1) / chunks;
  a.PS = 256 / a.CVt;
  a.npix = (long long)d.batch * d.tokens;
  a.momentum = d.momentum;
  a.eps = d.eps;
  r.L = d.tokens;
  r.x_lead = d.x_lead;
  r.y_lead = d.y_lead;
  r.rows_x = d.batch * (d.tokens + d.x_lead);
  r.rows_y = d.batch * (d.tokens + d.y_lead);
  r.dL = FDiv::make((unsigned)r.L);
  r.dLx = FDiv::make((unsigned)(r.L + r.x_lead));
  r.dLy = FDiv::make((unsigned)(r.L + r.y_lead));
  BnGrid g;
  g.chunks = chunks;
  g.sums = dw_blocks(a.npix, a.PS * kDwPix, std::max(128, std::min(kDwMaxBlocks, (4 << 20) / (16 * a.C))));
  g.apply = dw_blocks(r.rows_y, a.PS * kDwPix, 2 * kDwMaxBlocks);
  g.dx = dw_blocks(r.rows_x, a.PS * kDwPix, 2 * kDwMaxBlocks);
  return g;
}

size_t bn_workspace(int32_t B, int32_t L, int32_t C, int V) {
  sae_bnrows_desc d;
  memset(&d, 0, sizeof d);
  d.batch = B;
  d.tokens = L;
  d.channels = C;
  DwConvArgs a;
  BnRows r;
  return (size_t)bn_geometry(d, V, a, r).sums * 2 * C * sizeof(double);
}

// element offsets of x, y and lead rows must fit 31 bits (one more row per sample than tokens)
bool bn_extent_ok(long long B, long long L, long long C) { return B * (L + 1) * C <= 0x7fffffffLL; }

// everything but the pointers; every refusal returns before any HIP call
int bn_check(const char* what, const sae_bnrows_desc* d) {
  if (!d) return fail(SAE_EINVAL, "%s: NULL descriptor", what);
  if (d->batch < 1 || d->tokens < 1 || d->channels < 1)
    return fail(SAE_EUNSUPPORTED, "%s: batch %d, tokens %d, channels %d must be >= 1", what, d->batch, d->tokens, d->channels);
  if (d->dtype != SAE_DTYPE_BF16 && d->dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "%s: bad dtype %d", what, d->dtype);
  if ((d->x_lead != 0 && d->x_lead != 1) || (d->y_lead != 0 && d->y_lead != 1))
    return fail(SAE_EINVAL, "%s: x_lead %d, y_lead %d (0 or 1)", what, d->x_lead, d->y_lead);
  const int V = d->dtype == SAE_DTYPE_BF16 ? 8 : 4;
  if (d->channels % V)
    return fail(SAE_EUNSUPPORTED, "%s: channels %d must be a multiple of %d in %s", what, d->channels, V,
                d->dtype == SAE_DTYPE_BF16 ? "bf16" : "fp32");
  if (!bn_extent_ok(d->batch, d->tokens, d->channels))
    return fail(SAE_EUNSUPPORTED, "%s: element offsets exceed 2^31 - 1 (batch * (tokens + 1) * channels)", what);
  return SAE_OK;
}

template <typename T>
int bn_fwd_launch(hipStream_t st, const sae_bnrows_desc& d, DwConvArgs& a, BnRows& r) {
  const BnGrid g = bn_geometry(d, DwVec<T>::N, a, r);
  const dim3 gs((unsigned)g.sums, (unsigned)g.chunks), ga((unsigned)g.apply, (unsigned)g.chunks);
  if (!d.training) return launch("bn_gelu_eval", bn_rows_apply_kernel<T, false>, ga, dim3(256), 0, st, a, r);
  a.nparts = g.sums;
  if (int rc = launch("bn_gelu_stats", bn_rows_stats_kernel<T>, gs, dim3(256), 0, st, a, r)) return rc;
  if (int rc = launch("bn_gelu_stats_reduce", dwconv_reduce_kernel<double, true>, (long long)(a.C + kDwRedC - 1) / kDwRedC,
                      dim3(256), 0, st, a, a.C, (float*)nullptr, (float*)nullptr, 0))
    return rc;
  return launch("bn_gelu_apply", bn_rows_apply_kernel<T, true>, ga, dim3(256), 0, st, a, r);
}

template <typename T>
int bn_bwd_launch(hipStream_t st, const sae_bnrows_desc& d, DwConvArgs& a, BnRows& r) {
  const BnGrid g = bn_geometry(d, DwVec<T>::N, a, r);
  const dim3 gs((unsigned)g.sums, (unsigned)g.chunks), gx((unsigned)g.dx, (unsigned)g.chunks);
  a.nparts = g.sums;
  if (int rc = launch("bn_gelu_bwd_sums", bn_rows_bwd_sums_kernel<T>, gs, dim3(256), 0, st, a, r)) return rc;
  if (int rc = launch("bn_gelu_bwd_sums_reduce", dwconv_reduce_kernel<double, false>,
                      (long long)(2 * a.C + kDwRedC - 1) / kDwRedC, dim3(256), 0, st, a, 2 * a.C, a.dbeta, a.dgamma, a.C))
    return rc;
  return launch("bn_gelu_dx", bn_rows_dx_kernel<T>, gx, dim3(256), 0, st, a, r);
}

// ------------------------------------------- window matrix of the conv token embedding (CvT)
// Everything but the pointers, and the geometry of convtok.h; every refusal returns before any HIP
// call.  `gather`: in_dtype is read (the scatter has no x).
int ct_geometry(const char* what, const sae_convtok_desc* d, bool gather, ConvTokGeom& g) {
  if (!d) return fail(SAE_EINVAL, "%s: NULL descriptor", what);
  if (d->kernel < 1 || d->kernel > 7) return fail(SAE_EUNSUPPORTED, "%s: kernel %d (1..7)", what, d->kernel);
  if (d->stride < 1) return fail(SAE_EINVAL, "%s: stride %d must be >= 1", what, d->stride);
  if (d->batch < 1 || d->height < 1 || d->width < 1 || d->channels < 1)
    return fail(SAE_EINVAL, "%s: batch %d, height %d, width %d, channels %d must be >= 1", what, d->batch, d->height,
                d->width, d->channels);
  if (d->dtype != SAE_DTYPE_BF16 && d->dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "%s: bad dtype %d", what, d->dtype);
  if (gather && d->in_dtype != SAE_DTYPE_BF16 && d->in_dtype != SAE_DTYPE_F32)
    return fail(SAE_EINVAL, "%s: bad in_dtype %d", what, d->in_dtype);
  if (gather && d->in_dtype == SAE_DTYPE_BF16 && d->dtype == SAE_DTYPE_F32)
    return fail(SAE_EUNSUPPORTED, "%s: a bf16 x with an fp32 window matrix", what);
  const int k = d->kernel, s = d->stride;
  const long long Ho = ((long long)d->height + s - 1) / s, Wo = ((long long)d->width + s - 1) / s;
  const long long K = (long long)k * k * d->channels, Kp = (K + 7) / 8 * 8, M = d->batch * Ho * Wo;
  if ((long long)d->batch * d->height * d->width * d->channels > 0x7fffffffLL || M * Kp > 0x7fffffffLL)
    return fail(SAE_EUNSUPPORTED, "%s: element offsets exceed 2^31 - 1 (x %lld, window matrix %lld elements)", what,
                (long long)d->batch * d->height * d->width * d->channels, M * Kp);
  const int N = d->dtype == SAE_DTYPE_BF16 ? 8 : 4;
  g.B = d->batch;
  g.H = d->height;
  g.W = d->width;
  g.C = d->channels;
  g.k = k;
  g.s = s;
  g.Ho = (int)Ho;
  g.Wo = (int)Wo;
  g.pt = (int)std::max<long long>((Ho - 1) * s + k - g.H, 0) / 2;   // Flax SAME: the smaller half in front
  g.pl = (int)std::max<long long>((Wo - 1) * s + k - g.W, 0) / 2;
  g.K = (int)K;
  g.Kp = (int)Kp;
  g.M = (int)M;
  g.nch = g.Kp / N;
  g.total = g.M * g.nch;
  g.cch = (g.C + N - 1) / N;
  g.total_s = g.B * g.H * g.W * g.cch;   // (<= B H W C)
  g.dnch = FDiv::make((unsigned)g.nch);
  g.dHoWo = FDiv::make((unsigned)(g.Ho * g.Wo));
  g.dWo = FDiv::make((unsigned)g.Wo);
  g.dC = FDiv::make((unsigned)g.C);
  g.dk = FDiv::make((unsigned)k);
  g.dcch = FDiv::make((unsigned)g.cch);
  g.dHW = FDiv::make((unsigned)(g.H * g.W));
  g.dW = FDiv::make((unsigned)g.W);
  g.ds = FDiv::make((unsigned)s);
  return SAE_OK;
}

}  // namespace

extern "C" {

int sae_layernorm_fwd(void* stream, int32_t M, int32_t C, const float* x, const void* delta, float* xout,
                      const float* gamma, const float* beta, void* y, float* mean, float* rstd, float eps) {
  return ln_fwd_impl(stream, M, C, x, delta, xout, gamma, beta, y, mean, rstd, eps, nullptr, nullptr, 1);
}

int sae_layernorm_fwd_scaled(void* stream, int32_t M, int32_t C, const float* x, const void* delta, float* xout,
                             const float* gamma, const float* beta, void* y, float* mean, float* rstd, float eps,
                             const float* layerscale, const float* rowscale, int32_t rows_per_sample) {
  if (!delta || !layerscale) return fail(SAE_EINVAL, "layernorm_fwd_scaled: delta and layerscale are required");
  if (rowscale && (rows_per_sample < 1 || M % rows_per_sample))
    return fail(SAE_EINVAL, "layernorm_fwd_scaled: rows_per_sample (%d) must divide M (%d)", rows_per_sample, M);
  if (!aligned16(layerscale)) return fail(SAE_EINVAL, "layernorm_fwd_scaled: layerscale needs 16-byte alignment");
  return ln_fwd_impl(stream, M, C, x, delta, xout, gamma, beta, y, mean, rstd, eps, layerscale, rowscale,
                     rows_per_sample);
}

size_t sae_layernorm_bwd_workspace_bytes(int32_t M, int32_t C) {
  if (M < 1 || C < 1) return 0;
  return (size_t)ln_bwd_blocks(M) * 3 * C * sizeof(float);   // room for the scaled form
}

int sae_layernorm_bwd(void* stream, int32_t M, int32_t C, const float* x, const float* mean, const float* rstd,
                      const float* gamma, const void* dy, const float* dxin, float* dx, void* ddelta, float* dgamma,
                      float* dbeta, void* workspace) {
  return ln_bwd_impl(stream, M, C, x, mean, rstd, gamma, dy, dxin, dx, ddelta, dgamma, dbeta, workspace, nullptr,
                     nullptr, nullptr, 1, nullptr);
}

int sae_layernorm_bwd_scaled(void* stream, int32_t M, int32_t C, const float* x, const float* mean,
                             const float* rstd, const float* gamma, const void* dy, const float* dxin, float* dx,
                             void* ddelta, float* dgamma, float* dbeta, void* workspace, const void* delta,
                             const float* layerscale, const float* rowscale, int32_t rows_per_sample,
                             float* dlayerscale) {
  if (!delta || !layerscale || !dlayerscale)
    return fail(SAE_EINVAL, "layernorm_bwd_scaled: delta, layerscale and dlayerscale are required");
  if (rowscale && (rows_per_sample < 1 || M % rows_per_sample))
    return fail(SAE_EINVAL, "layernorm_bwd_scaled: rows_per_sample (%d) must divide M (%d)", rows_per_sample, M);
  if (!aligned16(layerscale) || ((uintptr_t)delta & 7))
    return fail(SAE_EINVAL, "layernorm_bwd_scaled: layerscale needs 16-byte, delta 8-byte alignment");
  return ln_bwd_impl(stream, M, C, x, mean, rstd, gamma, dy, dxin, dx, ddelta, dgamma, dbeta, workspace, delta,
                     layerscale, rowscale, rows_per_sample, dlayerscale);
}

int sae_tokens_fwd(void* stream, int32_t B, int32_t L, int32_t E, const void* tokens, const float* cls,
                   const float* pos, float* x) {
  return tokens_fwd_impl(stream, B, L, E, tokens, cls, pos, x, nullptr);
}

int sae_tokens_bwd(void* stream, int32_t B, int32_t L, int32_t E, const float* dx, void* dtokens, float* dcls,
                   float* dpos) {
  return tokens_bwd_impl(stream, B, L, E, dx, dtokens, dcls, dpos, nullptr);
}

// ------------------------------------------------------------------ hidden-state dropout
// Every entry point checks rate / rng / row_step first (no HIP call before), and forwards to the
// plain entry point when the rate quantises to T = 0.
int sae_dropout_rows(void* stream, int32_t M, int32_t C, int32_t dtype, const void* x, int64_t ldx, void* y,
                     int64_t ldy, float rate, const uint64_t* rng, uint32_t stream_id, int64_t row0,
                     int64_t row_step) {
  unsigned thr;
  if (int rc = rows_drop_check("dropout_rows", rate, rng, row_step, &thr)) return rc;
  if (dtype != SAE_DTYPE_BF16 && dtype != SAE_DTYPE_F32) return fail(SAE_EINVAL, "dropout_rows: bad dtype %d", dtype);
  if (M < 1 || C < 1 || ldx < C || ldy < C)
    return fail(SAE_EINVAL, "dropout_rows: M %d, C %d, ldx %lld, ldy %lld", M, C, (long long)ldx, (long long)ldy);
  if (!x || !y) return fail(SAE_EINVAL, "dropout_rows: x and y must be non-NULL");
  DropRowsArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.y = y;
  a.ldx = ldx;
  a.ldy = ldy;
  a.M = M;
  a.C = C;
  a.d = make_drop_rows(rng, stream_id, thr, row0, row_step);   // T = 0: every byte >= 0, inv = 1 -- a copy
  const uintptr_t amask = (uintptr_t)(4 * elem_size(dtype) - 1);
  a.vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && !((uintptr_t)x & amask) && !((uintptr_t)y & amask);
  const long long total = (long long)M * ((C + 3) / 4);
  const long long grid = std::min<long long>((total + 255) / 256, 16384);
  return by_dtype(dtype, [&](auto* t) {
    return launch("dropout_rows", dropout_rows_kernel<std::remove_pointer_t<decltype(t)>>, grid, dim3(256), 0,
                  (hipStream_t)stream, a);
  });
}

int sae_dropout_rows_mask(void* stream, int32_t M, int32_t C, float rate, const uint64_t* rng, uint32_t stream_id,
                          int64_t row0, int64_t row_step, uint8_t* keep) {
  unsigned thr;
  if (int rc = rows_drop_check("dropout_rows_mask", rate, rng, row_step, &thr)) return rc;
  if (M < 1 || C < 1 || !keep) return fail(SAE_EINVAL, "dropout_rows_mask: M %d, C %d, keep %p", M, C, (void*)keep);
  DropRowsArgs a;
  memset(&a, 0, sizeof a);
  a.keep = keep;
  a.M = M;
  a.C = C;
  a.d = make_drop_rows(rng, stream_id, thr, row0, row_step);
  return launch("dropout_rows_mask", dropout_rows_mask_kernel, ((long long)M * C + 255) / 256, dim3(256), 0,
                (hipStream_t)stream, a);
}

int sae_layernorm_fwd_dropout(void* stream, int32_t M, int32_t C, const float* x, const void* delta, float* xout,
                              const float* gamma, const float* beta, void* y, float* mean, float* rstd, float eps,
                              float rate, const uint64_t* rng, uint32_t stream_id, int64_t row0, int64_t row_step) {
  unsigned thr;
  if (int rc = rows_drop_check("layernorm_fwd_dropout", rate, rng, row_step, &thr)) return rc;
  if (!delta) return fail(SAE_EINVAL, "layernorm_fwd_dropout: delta is required");
  if (thr == 0) return sae_layernorm_fwd(stream, M, C, x, delta, xout, gamma, beta, y, mean, rstd, eps);
  const DropRows d = make_drop_rows(rng, stream_id, thr, row0, row_step);
  return ln_fwd_impl(stream, M, C, x, delta, xout, gamma, beta, y, mean, rstd, eps, nullptr, nullptr, 1, &d);
}

int sae_layernorm_bwd_dropout(void* stream, int32_t M, int32_t C, const float* x, const float* mean,
                              const float* rstd, const float* gamma, const void* dy, const float* dxin, float* dx,
                              void* ddelta, float* dgamma, float* dbeta, void* workspace, float rate,
                              const uint64_t* rng, uint32_t stream_id, int64_t row0, int64_t row_step) {
  unsigned thr;
  if (int rc = rows_drop_check("layernorm_bwd_dropout", rate, rng, row_step, &thr)) return rc;
  if (thr == 0) return sae_layernorm_bwd(stream, M, C, x, mean, rstd, gamma, dy, dxin, dx, ddelta, dgamma, dbeta, workspace);
  const DropRows d = make_drop_rows(rng, stream_id, thr, row0, row_step);
  return ln_bwd_impl(stream, M, C, x, mean, rstd, gamma, dy, dxin, dx, ddelta, dgamma, dbeta, workspace, nullptr,
                     nullptr, nullptr, 1, nullptr, &d);
}

int sae_tokens_fwd_dropout(void* stream, int32_t B, int32_t L, int32_t E, const void* tokens, const float* cls,
                           const float* pos, float* x, float rate, const uint64_t* rng, uint32_t stream_id) {
  unsigned thr;
  if (int rc = rows_drop_check("tokens_fwd_dropout", rate, rng, 1, &thr)) return rc;
  if (thr == 0) return sae_tokens_fwd(stream, B, L, E, tokens, cls, pos, x);
  const DropRows d = make_drop_rows(rng, stream_id, thr, 0, 1);
  return tokens_fwd_impl(stream, B, L, E, tokens, cls, pos, x, &d);
}

int sae_tokens_bwd_dropout(void* stream, int32_t B, int32_t L, int32_t E, const float* dx, void* dtokens, float* dcls,
                           float* dpos, float rate, const uint64_t* rng, uint32_t stream_id) {
  unsigned thr;
  if (int rc = rows_drop_check("tokens_bwd_dropout", rate, rng, 1, &thr)) return rc;
  if (thr == 0) return sae_tokens_bwd(stream, B, L, E, dx, dtokens, dcls, dpos);
  const DropRows d = make_drop_rows(rng, stream_id, thr, 0, 1);
  return tokens_bwd_impl(stream, B, L, E, dx, dtokens, dcls, dpos, &d);
}

// the loss family (ce_fwd_impl / ce_bwd_impl); sae_smoothed_ce_* is sae_mixed_ce_* with the optional arguments NULL
int sae_mixed_ce_fwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld, int32_t dtype,
                     const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha, float* lse,
                     float* row_loss, int32_t* rank, float* loss, float* top) {
  return ce_fwd_impl("mixed_ce_fwd", stream, rows, classes, logits, ld, dtype, labels, mix_labels, ratio, alpha, lse,
                     row_loss, rank, loss, top);
}

int sae_mixed_ce_bwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld, int32_t dtype,
                     const int64_t* labels, const int64_t* mix_labels, const float* ratio, float alpha,
                     const float* lse, const float* grad_loss, void* dlogits, int64_t ldd) {
  return ce_bwd_impl("mixed_ce_bwd", stream, rows, classes, logits, ld, dtype, labels, mix_labels, ratio, alpha, lse,
                     grad_loss, dlogits, ldd);
}

int sae_smoothed_ce_fwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                        int32_t dtype, const int64_t* labels, float alpha, float* lse, float* row_loss, float* loss) {
  return ce_fwd_impl("smoothed_ce_fwd", stream, rows, classes, logits, ld, dtype, labels, nullptr, nullptr, alpha, lse,
                     row_loss, nullptr, loss, nullptr);
}

int sae_smoothed_ce_bwd(void* stream, int32_t rows, int32_t classes, const void* logits, int64_t ld,
                        int32_t dtype, const int64_t* labels, float alpha, const float* lse,
                        const float* grad_loss, void* dlogits, int64_t ldd) {
  return ce_bwd_impl("smoothed_ce_bwd", stream, rows, classes, logits, ld, dtype, labels, nullptr, nullptr, alpha, lse,
                     grad_loss, dlogits, ldd);
}

static_assert(sizeof(CeAccum) == SAE_CE_ACCUM_BYTES, "the evaluation accumulator is 32 bytes");

int sae_ce_accumulate(void* stream, int32_t rows, const float* row_loss, const int32_t* rank, void* acc) {
  if (rows < 1 || rows > SAE_CE_MAX_ROWS)
    return fail(SAE_EINVAL, "ce_accumulate: rows %d (1..%d)", rows, SAE_CE_MAX_ROWS);
  if (!row_loss || !rank || !acc) return fail(SAE_EINVAL, "ce_accumulate: NULL row_loss / rank / acc");
  if ((uintptr_t)acc & 7) return fail(SAE_EINVAL, "ce_accumulate: acc must be 8-byte aligned");
  return launch("ce_accumulate", ce_accumulate_kernel, 1LL, dim3(256), 0, (hipStream_t)stream, row_loss,
                (const int*)rank, rows, reinterpret_cast<CeAccum*>(acc));
}

// ------------------------------------------------- depthwise 3x3 convolution + BatchNorm (CvT)
size_t sae_dwconv_bn_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || C % 4 || (stride != 1 && stride != 2) || (long long)B * H * W > (1LL << 30))
    return 0;
  sae_dwconv_desc d;
  memset(&d, 0, sizeof d);
  d.batch = B;
  d.height = H;
  d.width = W;
  d.channels = C;
  d.stride = stride;
  return std::max(dw_workspace(d, 4), C % 8 ? (size_t)0 : dw_workspace(d, 8));   // either element type
}

int sae_dwconv_bn_fwd(void* stream, const sae_dwconv_desc* desc, const void* x, const float* w, const float* gamma,
                      const float* beta, float* run_mean, float* run_var, void* t, void* y, float* mean, float* rstd,
                      void* workspace) {
  if (int rc = dw_check("dwconv_bn_fwd", desc)) return rc;
  if (!x || !w || !gamma || !beta || !run_mean || !run_var || !y)
    return fail(SAE_EINVAL, "dwconv_bn_fwd: NULL x / w / gamma / beta / run_mean / run_var / y");
  if (desc->training && (!t || !mean || !rstd || !workspace))
    return fail(SAE_EINVAL, "dwconv_bn_fwd: training needs t, mean, rstd and workspace");
  if (!aligned16(x) || !aligned16(w) || !aligned16(gamma) || !aligned16(beta) || !aligned16(run_mean) ||
      !aligned16(run_var) || !aligned16(t) || !aligned16(y) || !aligned16(mean) || !aligned16(rstd) ||
      !aligned16(workspace))
    return fail(SAE_EINVAL, "dwconv_bn_fwd: every pointer needs 16-byte alignment");
  DwConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.w = w;
  a.gamma = gamma;
  a.beta = beta;
  a.run_mean = run_mean;
  a.run_var = run_var;
  a.t = t;
  a.y = y;
  a.mean = mean;
  a.rstd = rstd;
  a.part = workspace;
  return by_dtype(desc->dtype, [&](auto* p) {
    return dw_fwd_launch<std::remove_pointer_t<decltype(p)>>((hipStream_t)stream, *desc, a);
  });
}

int sae_dwconv_bn_bwd(void* stream, const sae_dwconv_desc* desc, const void* x, const float* w, const float* gamma,
                      const void* t, const float* mean, const float* rstd, const void* dy, void* dx, float* dw,
                      float* dgamma, float* dbeta, void* workspace) {
  if (int rc = dw_check("dwconv_bn_bwd", desc)) return rc;
  if (!desc->training)
    return fail(SAE_EUNSUPPORTED, "dwconv_bn_bwd: training = 0 (the evaluation form has no backward)");
  if (!x || !w || !gamma || !t || !mean || !rstd || !dy || !dx || !dw || !dgamma || !dbeta || !workspace)
    return fail(SAE_EINVAL, "dwconv_bn_bwd: NULL argument");
  if (!aligned16(x) || !aligned16(w) || !aligned16(gamma) || !aligned16(t) || !aligned16(mean) || !aligned16(rstd) ||
      !aligned16(dy) || !aligned16(dx) || !aligned16(dw) || !aligned16(dgamma) || !aligned16(dbeta) ||
      !aligned16(workspace))
    return fail(SAE_EINVAL, "dwconv_bn_bwd: every pointer needs 16-byte alignment");
  DwConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.w = w;
  a.gamma = gamma;
  a.t = const_cast<void*>(t);
  a.mean = const_cast<float*>(mean);
  a.rstd = const_cast<float*>(rstd);
  a.dy = dy;
  a.dx = dx;
  a.dw = dw;
  a.dgamma = dgamma;
  a.dbeta = dbeta;
  a.part = workspace;
  return by_dtype(desc->dtype, [&](auto* p) {
    return dw_bwd_launch<std::remove_pointer_t<decltype(p)>>((hipStream_t)stream, *desc, a);
  });
}

// ------------------------------------------------- BatchNorm + GELU over token rows (CeiT LeFF)
size_t sae_bn_gelu_workspace_bytes(int32_t B, int32_t L, int32_t C) {
  if (B < 1 || L < 1 || C < 1 || C % 4 || !bn_extent_ok(B, L, C)) return 0;
  return std::max(bn_workspace(B, L, C, 4), C % 8 ? (size_t)0 : bn_workspace(B, L, C, 8));   // either element type
}

int sae_bn_gelu_fwd(void* stream, const sae_bnrows_desc* desc, const void* x, const float* gamma, const float* beta,
                    float* run_mean, float* run_var, const void* lead, int64_t lead_pitch, void* y, float* mean,
                    float* rstd, void* workspace) {
  if (int rc = bn_check("bn_gelu_fwd", desc)) return rc;
  if (!x || !gamma || !beta || !run_mean || !run_var || !y)
    return fail(SAE_EINVAL, "bn_gelu_fwd: NULL x / gamma / beta / run_mean / run_var / y");
  if (desc->training && (!mean || !rstd || !workspace))
    return fail(SAE_EINVAL, "bn_gelu_fwd: training needs mean, rstd and workspace");
  const int V = desc->dtype == SAE_DTYPE_BF16 ? 8 : 4;
  if (desc->y_lead) {
    if (!lead) return fail(SAE_EINVAL, "bn_gelu_fwd: y_lead = 1 needs lead");
    if (lead_pitch < 0 || lead_pitch % V)
      return fail(SAE_EUNSUPPORTED, "bn_gelu_fwd: lead_pitch %lld must be a non-negative multiple of %d", (long long)lead_pitch, V);
    if ((long long)(desc->batch - 1) * lead_pitch + desc->channels > 0x7fffffffLL)
      return fail(SAE_EUNSUPPORTED, "bn_gelu_fwd: lead element offsets exceed 2^31 - 1");
  }
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(run_mean) || !aligned16(run_var) ||
      !aligned16(lead) || !aligned16(y) || !aligned16(mean) || !aligned16(rstd) || !aligned16(workspace))
    return fail(SAE_EUNSUPPORTED, "bn_gelu_fwd: every pointer needs 16-byte alignment");
  DwConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.run_mean = run_mean;
  a.run_var = run_var;
  a.y = y;
  a.mean = mean;
  a.rstd = rstd;
  a.part = workspace;
  BnRows r;
  memset(&r, 0, sizeof r);
  r.lead = desc->y_lead ? lead : x;   // (never read without y_lead)
  r.lead_pitch = desc->y_lead ? lead_pitch : 0;
  return by_dtype(desc->dtype, [&](auto* p) {
    return bn_fwd_launch<std::remove_pointer_t<decltype(p)>>((hipStream_t)stream, *desc, a, r);
  });
}

int sae_bn_gelu_bwd(void* stream, const sae_bnrows_desc* desc, const void* x, const float* gamma, const float* beta,
                    const float* mean, const float* rstd, const void* dy, void* dx, float* dgamma, float* dbeta,
                    void* workspace) {
  if (int rc = bn_check("bn_gelu_bwd", desc)) return rc;
  if (!desc->training)
    return fail(SAE_EUNSUPPORTED, "bn_gelu_bwd: training = 0 (the evaluation form has no backward)");
  if (!x || !gamma || !beta || !mean || !rstd || !dy || !dx || !dgamma || !dbeta || !workspace)
    return fail(SAE_EINVAL, "bn_gelu_bwd: NULL argument");
  if (!aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(mean) || !aligned16(rstd) || !aligned16(dy) ||
      !aligned16(dx) || !aligned16(dgamma) || !aligned16(dbeta) || !aligned16(workspace))
    return fail(SAE_EUNSUPPORTED, "bn_gelu_bwd: every pointer needs 16-byte alignment");
  DwConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x;
  a.gamma = gamma;
  a.beta = beta;
  a.mean = const_cast<float*>(mean);
  a.rstd = const_cast<float*>(rstd);
  a.dy = dy;
  a.dx = dx;
  a.dgamma = dgamma;
  a.dbeta = dbeta;
  a.part = workspace;
  BnRows r;
  memset(&r, 0, sizeof r);
  return by_dtype(desc->dtype, [&](auto* p) {
    return bn_bwd_launch<std::remove_pointer_t<decltype(p)>>((hipStream_t)stream, *desc, a, r);
  });
}

// ------------------------------------------- window matrix of the conv token embedding (CvT)
int32_t sae_conv_window_cols(int32_t channels, int32_t kernel) {
  if (channels < 1 || kernel < 1 || kernel > 7) return 0;
  const long long Kp = ((long long)kernel * kernel * channels + 7) / 8 * 8;
  return Kp > 0x7fffffffLL ? 0 : (int32_t)Kp;
}

int sae_conv_window_gather(void* stream, const sae_convtok_desc* desc, const void* x, void* P) {
  ConvTokGeom g;
  if (int rc = ct_geometry("conv_window_gather", desc, true, g)) return rc;
  if (!x || !P) return fail(SAE_EINVAL, "conv_window_gather: NULL x / P");
  const bool bf = desc->dtype == SAE_DTYPE_BF16, xbf = desc->in_dtype == SAE_DTYPE_BF16;
  const bool vec = g.C % (bf ? 8 : 4) == 0;
  if (!aligned16(P) || (vec && !aligned16(x)) || ((uintptr_t)x & (xbf ? 1 : 3)))
    return fail(SAE_EINVAL, "conv_window_gather: P (and x on the 16-byte path) needs 16-byte alignment");
  const long long grid = ((long long)g.total + 255) / 256;
  hipStream_t st = (hipStream_t)stream;
  if (!bf)
    return launch("conv_window_gather", vec ? conv_window_gather_kernel<float, float, true>
                                            : conv_window_gather_kernel<float, float, false>,
                  grid, dim3(256), 0, st, g, reinterpret_cast<const float*>(x), reinterpret_cast<float*>(P));
  if (xbf)
    return launch("conv_window_gather", vec ? conv_window_gather_kernel<__bf16, __bf16, true>
                                            : conv_window_gather_kernel<__bf16, __bf16, false>,
                  grid, dim3(256), 0, st, g, reinterpret_cast<const __bf16*>(x), reinterpret_cast<__bf16*>(P));
  return launch("conv_window_gather", vec ? conv_window_gather_kernel<float, __bf16, true>
                                          : conv_window_gather_kernel<float, __bf16, false>,
                grid, dim3(256), 0, st, g, reinterpret_cast<const float*>(x), reinterpret_cast<__bf16*>(P));
}

int sae_conv_window_scatter(void* stream, const sae_convtok_desc* desc, const void* dP, void* dX) {
  ConvTokGeom g;
  if (int rc = ct_geometry("conv_window_scatter", desc, false, g)) return rc;
  if (!dP || !dX) return fail(SAE_EINVAL, "conv_window_scatter: NULL dP / dX");
  const bool bf = desc->dtype == SAE_DTYPE_BF16;
  const bool vec = g.C % (bf ? 8 : 4) == 0;
  if (!aligned16(dP) || (vec && !aligned16(dX)) || ((uintptr_t)dX & (bf ? 1 : 3)))
    return fail(SAE_EINVAL, "conv_window_scatter: dP (and dX on the 16-byte path) needs 16-byte alignment");
  const long long grid = ((long long)g.total_s + 255) / 256;
  return by_dtype(desc->dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    return launch("conv_window_scatter", vec ? conv_window_scatter_kernel<T, true> : conv_window_scatter_kernel<T, false>,
                  grid, dim3(256), 0, (hipStream_t)stream, g, reinterpret_cast<const T*>(dP), reinterpret_cast<T*>(dX));
  });
}


// ---------------------------------------------------------------------------------- AdamW
static_assert(sizeof(sae_adamw_chunk) == sizeof(AdamwChunk) && SAE_ADAMW_CHUNK == kAdamwChunk,
              "sae_adamw_chunk mirrors AdamwChunk");

int sae_adamw_plan(int32_t n_items, float* const* p, const float* const* g, float* const* m, float* const* v,
                   const int64_t* n, sae_adamw_chunk* chunks, int64_t max_chunks, int64_t* n_chunks) {
  if (n_items < 0 || !n_chunks || (n_items > 0 && (!p || !g || !m || !v || !n)))
    return fail(SAE_EINVAL, "adamw_plan: bad arguments");
  int64_t k = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    if (n[i] < 0 || (n[i] > 0 && (!p[i] || !g[i] || !m[i] || !v[i])))
      return fail(SAE_EINVAL, "adamw_plan: item %d invalid", i);
    for (int64_t off = 0; off < n[i]; off += SAE_ADAMW_CHUNK, ++k) {
      if (k < max_chunks && chunks) {
        sae_adamw_chunk& c = chunks[k];
        c.p = p[i] + off;
        c.g = g[i] + off;
        c.m = m[i] + off;
        c.v = v[i] + off;
        c.n = (int32_t)std::min<int64_t>(SAE_ADAMW_CHUNK, n[i] - off);
        c.vec = c.n == SAE_ADAMW_CHUNK && aligned16(c.p) && aligned16(c.g) && aligned16(c.m) && aligned16(c.v);
      }
    }
  }
  *n_chunks = k;
  if (k > max_chunks) return fail(SAE_EINVAL, "adamw_plan: %lld chunks > capacity %lld", (long long)k,
                                  (long long)max_chunks);
  return ok();
}

int sae_adamw_step(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int32_t* step, float lr,
                   float beta1, float beta2, float eps, float weight_decay) {
  if (n_chunks < 0 || n_chunks >= (1LL << 31) || (n_chunks > 0 && !chunks) || !step)
    return fail(SAE_EINVAL, "adamw_step: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch("adamw_tick", adamw_tick_kernel, 1LL, dim3(64), 0, st, step)) return rc;
  if (n_chunks == 0) return ok();
  return launch("adamw", adamw_kernel, (long long)n_chunks, dim3(256), 0, st, reinterpret_cast<const AdamwChunk*>(chunks),
                step, lr, beta1, beta2, eps, weight_decay);
}

static_assert(sizeof(sae_adamw_cast_tile) == sizeof(AdamwCastTile), "sae_adamw_cast_tile mirrors AdamwCastTile");

int sae_adamw_cast_plan(int32_t n_items, float* const* p, const float* const* g, float* const* m,
                        float* const* v, const int32_t* K, const int32_t* N, void* const* w16, const int32_t* ld16,
                        void* const* wt16, const int32_t* ldT, const int32_t* col0, sae_adamw_cast_tile* tiles,
                        int64_t max_tiles, int64_t* n_tiles) {
  if (n_items < 0 || !n_tiles || (n_items > 0 && (!p || !g || !m || !v || !K || !N || !col0)))
    return fail(SAE_EINVAL, "adamw_cast_plan: bad arguments");
  const auto a8 = [](const void* q) { return ((uintptr_t)q & 7) == 0; };
  int64_t k = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    void* o16 = w16 ? w16[i] : nullptr;
    void* oT = wt16 ? wt16[i] : nullptr;
    const int32_t l16 = ld16 ? ld16[i] : 0, lT = ldT ? ldT[i] : 0;
    if (!p[i] || !g[i] || !m[i] || !v[i] || K[i] < 1 || N[i] < 1 || col0[i] < 0 || (!o16 && !oT) ||
        (o16 && l16 < col0[i] + N[i]) || (oT && lT < K[i]))
      return fail(SAE_EINVAL, "adamw_cast_plan: item %d invalid (K %d N %d col0 %d ld16 %d ldT %d)", i, K[i], N[i],
                  col0[i], l16, lT);
    if (K[i] % 4 || N[i] % 4 || col0[i] % 4 || !aligned16(p[i]) || !aligned16(g[i]) || !aligned16(m[i]) ||
        !aligned16(v[i]) || (o16 && (l16 % 4 || !a8(o16))) || (oT && (lT % 4 || !a8(oT))))
      return fail(SAE_EUNSUPPORTED, "adamw_cast_plan: item %d needs K/N/col0/ld multiples of 4 and aligned buffers",
                  i);
    for (int32_t k0 = 0; k0 < K[i]; k0 += 64)
      for (int32_t n0 = 0; n0 < N[i]; n0 += 64, ++k) {
        if (k < max_tiles && tiles) {
          sae_adamw_cast_tile& t = tiles[k];
          t.p = p[i];
          t.g = g[i];
          t.m = m[i];
          t.v = v[i];
          t.w16 = o16;
          t.wt16 = oT;
          t.K = K[i];
          t.N = N[i];
          t.ld16 = l16;
          t.ldT = lT;
          t.col0 = col0[i];
          t.k0 = k0;
          t.n0 = n0;
          t.pad = 0;
        }
      }
  }
  *n_tiles = k;
  if (k > max_tiles)
    return fail(SAE_EINVAL, "adamw_cast_plan: %lld tiles > capacity %lld", (long long)k, (long long)max_tiles);
  return ok();
}

int sae_adamw_step_cast(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int64_t n_tiles,
                        const sae_adamw_cast_tile* tiles, int32_t* step, float lr, float beta1, float beta2, float eps,
                        float weight_decay) {
  if (n_chunks < 0 || n_tiles < 0 || n_chunks + n_tiles >= (1LL << 31) || (n_chunks > 0 && !chunks) ||
      (n_tiles > 0 && !tiles) || !step)
    return fail(SAE_EINVAL, "adamw_step_cast: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch("adamw_tick", adamw_tick_kernel, 1LL, dim3(64), 0, st, step)) return rc;
  if (n_chunks + n_tiles == 0) return ok();
  return launch("adamw_cast", adamw_cast_kernel, (long long)(n_chunks + n_tiles), dim3(256), 0, st,
                reinterpret_cast<const AdamwChunk*>(chunks), (int)n_chunks, reinterpret_cast<const AdamwCastTile*>(tiles),
                step, lr, beta1, beta2, eps, weight_decay);
}

// ---- the reference's chain around the update: global-norm clip and learning-rate schedule
static_assert(sizeof(sae_lr_schedule) == sizeof(AdamwSchedule) && SAE_ADAMW_NORM_SPAN == kAdamwNormSpan &&
                  SAE_ADAMW_PREPARE_PASS == kAdamwPreparePass && SAE_LR_CONSTANT == 0,
              "sae_lr_schedule mirrors AdamwSchedule");

// x is a finite number >= lo (> lo if strict); +inf passes if inf_ok.  NaN is tested on the bits:
// the library is compiled with -fno-honor-nans, under which a comparison may not refuse one.
static bool adamw_arg_ok(float x, float lo, bool strict, bool inf_ok) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  if ((u & 0x7fffffffu) > 0x7f800000u) return false;
  if (!inf_ok && (u & 0x7fffffffu) == 0x7f800000u) return false;
  return strict ? x > lo : x >= lo;
}

size_t sae_adamw_prepare_workspace_bytes(int64_t n) {
  return n < 1 ? 0 : (size_t)((n + SAE_ADAMW_NORM_SPAN - 1) / SAE_ADAMW_NORM_SPAN) * sizeof(double);
}

int sae_adamw_prepare(void* stream, int64_t n, const float* g, float max_norm, const sae_lr_schedule* schedule,
                      int32_t* step, void* workspace, float* hyper) {
  if (!schedule || !step || !hyper) return fail(SAE_EINVAL, "adamw_prepare: NULL schedule / step / hyper");
  const bool with_norm = n != 0 || g || workspace;   // n == 0 and both NULL: the schedule alone
  if (with_norm && (n < 1 || !g || !workspace))
    return fail(SAE_EINVAL, "adamw_prepare: the norm pass needs n >= 1 (%lld), g and workspace", (long long)n);
  if (with_norm && (((uintptr_t)g & 3) || ((uintptr_t)workspace & 7)))
    return fail(SAE_EINVAL, "adamw_prepare: g must be 4-byte and workspace 8-byte aligned");
  if (!adamw_arg_ok(max_norm, 0.f, true, true))
    return fail(SAE_EINVAL, "adamw_prepare: max_norm (%g) must be > 0 (+inf: no clip)", (double)max_norm);
  const sae_lr_schedule& s = *schedule;
  if (s.kind != SAE_LR_CONSTANT && s.kind != SAE_LR_WARMUP_COSINE)
    return fail(SAE_EINVAL, "adamw_prepare: unknown schedule kind %d", s.kind);
  if (!adamw_arg_ok(s.peak, 0.f, true, false))
    return fail(SAE_EINVAL, "adamw_prepare: peak (%g) must be > 0 and finite", (double)s.peak);
  if (s.kind == SAE_LR_WARMUP_COSINE) {
    if (s.warmup_steps < 0) return fail(SAE_EINVAL, "adamw_prepare: warmup_steps (%d) must be >= 0", s.warmup_steps);
    if (s.decay_steps <= s.warmup_steps)
      return fail(SAE_EINVAL, "adamw_prepare: decay_steps (%d) must be > warmup_steps (%d)", s.decay_steps,
                  s.warmup_steps);
    if (!adamw_arg_ok(s.init, 0.f, false, false) || !adamw_arg_ok(s.end, 0.f, false, false))
      return fail(SAE_EINVAL, "adamw_prepare: init (%g) and end (%g) must be >= 0 and finite", (double)s.init,
                  (double)s.end);
  }
  hipStream_t st = (hipStream_t)stream;
  const long long parts = with_norm ? (long long)((n + SAE_ADAMW_NORM_SPAN - 1) / SAE_ADAMW_NORM_SPAN) : 0;
  if (parts > 0x7fffffffLL) return fail(SAE_EUNSUPPORTED, "adamw_prepare: n %lld too large", (long long)n);
  double* partial = reinterpret_cast<double*>(workspace);
  if (with_norm)
    if (int rc = launch("adamw_sumsq", adamw_sumsq_kernel, parts, dim3(256), 0, st, g, (long long)n, partial)) return rc;
  AdamwSchedule k;
  memcpy(&k, &s, sizeof k);
  return launch("adamw_prepare", adamw_prepare_kernel, 1LL, dim3(256), 0, st, (const double*)partial, (int)parts,
                max_norm, k, step, hyper);
}

int sae_adamw_step_dev(void* stream, int64_t n_chunks, const sae_adamw_chunk* chunks, int64_t n_tiles,
                       const sae_adamw_cast_tile* tiles, const int32_t* step, const float* hyper, float beta1,
                       float beta2, float eps, float weight_decay) {
  if (n_chunks < 0 || n_tiles < 0 || n_chunks + n_tiles >= (1LL << 31) || (n_chunks > 0 && !chunks) ||
      (n_tiles > 0 && !tiles) || !step || !hyper)
    return fail(SAE_EINVAL, "adamw_step_dev: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (n_chunks + n_tiles == 0) return ok();
  if (n_tiles == 0)
    return launch("adamw_dev", adamw_dev_kernel, (long long)n_chunks, dim3(256), 0, st,
                  reinterpret_cast<const AdamwChunk*>(chunks), step, hyper, beta1, beta2, eps, weight_decay);
  return launch("adamw_cast_dev", adamw_cast_dev_kernel, (long long)(n_chunks + n_tiles), dim3(256), 0, st,
                reinterpret_cast<const AdamwChunk*>(chunks), (int)n_chunks, reinterpret_cast<const AdamwCastTile*>(tiles),
                step, hyper, beta1, beta2, eps, weight_decay);
}

// ------------------------------------------------------------------------ stream utilities
// bench.py --emulate-rccl: workgroups that hold their CU's slots (waves, LDS) for `ticks` of the
// 100 MHz real-time counter while sleeping -- the CU footprint of an RCCL ring channel
__global__ void occupy_cus_kernel(long long ticks) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const long long t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) lds[0] = 0;
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

__global__ void flag_bump_kernel(unsigned* flag) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int sae_occupy_cus(void* stream, int32_t workgroups, int32_t threads, int32_t lds_bytes, float usec) {
  if (workgroups < 1 || threads < 64 || threads > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024 || !(usec >= 0.f))
    return fail(SAE_EINVAL, "occupy_cus: bad arguments (%d workgroups, %d threads, %d B LDS, %g us)", workgroups,
                threads, lds_bytes, (double)usec);
  return launch("occupy_cus", occupy_cus_kernel, (long long)workgroups, dim3((unsigned)threads), (size_t)lds_bytes,
                (hipStream_t)stream, (long long)(usec * 100.f));
}

int sae_flag_bump(void* stream, uint32_t* flags, int32_t index) {
  if (!flags || index < 0) return fail(SAE_EINVAL, "flag_bump: flags must be non-NULL and index >= 0");
  return launch("flag_bump", flag_bump_kernel, 1LL, dim3(64), 0, (hipStream_t)stream, (unsigned*)flags + index);
}

int sae_stream_wait_flag(void* stream, const uint32_t* flag, uint32_t value) {
  if (!flag || ((uintptr_t)flag & 3)) return fail(SAE_EINVAL, "stream_wait_flag: flag must be a non-NULL 4-byte-aligned pointer");
  const hipError_t e = hipStreamWaitValue32((hipStream_t)stream, const_cast<uint32_t*>(flag), value,
                                            hipStreamWaitValueGte, 0xffffffffu);
  if (e != hipSuccess) return fail(SAE_EHIP, "hipStreamWaitValue32: %s", hipGetErrorString(e));
  return ok();
}

// ------------------------------------------------------------------------------ the library
const char* sae_last_error(void) { return g_err.c_str(); }

int32_t sae_abi_version(void) { return SAE_ABI_VERSION; }

const char* sae_build_info(void) { return "sae_attn gfx950 (" __DATE__ " " __TIME__ ")"; }

}  // extern "C"

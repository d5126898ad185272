// dwconv.h -- the CvT convolutional projection in front of the 1x1 GEMM: depthwise 3x3 convolution
// (stride 1 or 2, Flax SAME padding) + BatchNorm, forward and backward.
//
// Reference: models/layers/attentions/cvt_attention.py:12-40.  x [B][H][W][C] in the compute dtype
// T (bf16 or fp32), depthwise kernel w fp32 [3][3][C] used at T (rounded as it is loaded, like the
// LayerScale parameter of ln.h), Ho = ceil(H / s), total padding max((Ho - 1) s + 3 - H, 0) with the
// smaller half in front (pt, pl):
//     t[b,p,q,c] = T( sum_{i,j} xp[b, p s + i, q s + j, c] w[i,j,c] )    fp32, i outer, j inner
//     training:   mu, var = biased batch statistics of t (fp64 sums of the T-rounded values),
//                 r = rsqrt(var + eps), y = T( ((t - mu) r) gamma + beta ),
//                 run_mean = m run_mean + (1 - m) mu, run_var = m run_var + (1 - m) var
//     evaluation: the same formula with run_mean / run_var, one kernel, buffers untouched
//     backward:   dbeta = sum g, dgamma = sum g xhat, dt = gamma r (g - dbeta / N - xhat dgamma / N),
//                 dw[i,j,c] = sum xp dt, dx by gather over the taps of dt rounded to T
//
// Layout.  The channel vector (16 bytes: 8 bf16 or 4 fp32) is innermost on the lanes: a workgroup's
// 256 threads are PS pixel slots x CVt channel vectors (CVt = min(C / V, 256); thread = slot * CVt +
// vector), so a wave's loads are runs of consecutive 16-byte chunks of one pixel and every thread
// keeps one channel vector for its whole life -- its 9 weights, its statistics and its BatchNorm
// constants stay in registers.  A slot walks runs of kDwRun output pixels along W and keeps the
// 3-row window of such a run in registers; the parallelism is over pixels, so C = 64 fills the chip.
//
// Reductions.  No floating-point atomics: every per-channel sum is a per-thread partial (fp64 for
// the statistics and for dbeta / dgamma, fp32 for dw), summed over the slots of a workgroup through
// LDS in slot order, written as a per-workgroup partial row and summed over the workgroups in index
// order by dwconv_reduce_kernel.  Two runs give the same bits.  The batch statistics are fp64 sums
// of t and t^2 (t has at most 24 significant bits, so t^2 is exact in fp64): var = E[t^2] - mu^2 does
// not cancel for inputs with a large mean the way fp32 sums would.
#pragma once
#include "common.h"

namespace sae {

constexpr int kDwRun = 4;       // output pixels a lane walks along W (a multiple of 2)
constexpr int kDwPix = 4;       // pixels in flight per lane in the per-pixel passes
constexpr int kDwRedS = 32;     // slices a column's partials are summed in (dwconv_reduce_kernel)
constexpr int kDwRedC = 8;      // columns per workgroup there (kDwRedS * kDwRedC = 256 threads)

struct DwConvArgs {
  const void* x;          // [B][H][W][C] T
  const float* w;         // [3][3][C] fp32
  const float* gamma;     // [C]
  const float* beta;      // [C]
  float* run_mean;        // [C] running statistics (training: updated; evaluation: read)
  float* run_var;         // [C]
  void* t;                // [B][Ho][Wo][C] T conv output (training)
  void* y;                // [B][Ho][Wo][C] T
  float* mean;            // [C] batch mean (training)
  float* rstd;            // [C]
  const void* dy;         // [B][Ho][Wo][C] T
  void* dx;               // [B][H][W][C] T
  float* dw;              // [3][3][C]
  float* dgamma;          // [C]
  float* dbeta;           // [C]
  void* part;             // workspace: per-workgroup partial rows
  void* dt;               // workspace: [B][Ho][Wo][C] T gradient of t (dw kernel -> dx kernel)
  int B, H, W, C, Ho, Wo, pt, pl;
  int CVt, PS;            // channel vectors and pixel slots per workgroup
  int nruns, rpr;         // runs of kDwRun output pixels (B * Ho * rpr), runs per output row
  int nruns_in, rpr_in;   // the same over the input grid (dx)
  long long npix;         // B * Ho * Wo
  int nparts;             // partial rows the reduce kernel sums
  float momentum, eps;
};

template <typename T> struct DwVec;
template <> struct DwVec<__bf16> {
  static constexpr int N = 8;
  using raw = bf16x8;
};
template <> struct DwVec<float> {
  static constexpr int N = 4;
  using raw = f32x4;
};

template <typename T>
__device__ __forceinline__ typename DwVec<T>::raw dw_ld(const T* p, bool ok) {
  typename DwVec<T>::raw r = {};
  if (ok) r = *reinterpret_cast<const typename DwVec<T>::raw*>(p);
  return r;
}

template <typename T>
__device__ __forceinline__ void dw_st(T* p, const float (&v)[DwVec<T>::N]) {
  typename DwVec<T>::raw r;
#pragma unroll
  for (int e = 0; e < DwVec<T>::N; ++e) r[e] = (T)v[e];
  *reinterpret_cast<typename DwVec<T>::raw*>(p) = r;
}

// V consecutive fp32 parameters (16-byte aligned: the host checks the base, V is a multiple of 4)
template <int V>
__device__ __forceinline__ void dw_ldf(const float* p, float (&v)[V]) {
#pragma unroll
  for (int k = 0; k < V / 4; ++k) {
    const f32x4 r = reinterpret_cast<const f32x4*>(p)[k];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * k + e] = r[e];
  }
}

// the 9 taps of a thread's channel vector at the compute dtype
template <typename T, int V>
__device__ __forceinline__ void dw_taps(const float* w, int C, int c0, float (&wt)[9][V]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    dw_ldf<V>(w + (long long)k * C + c0, wt[k]);
#pragma unroll
    for (int e = 0; e < V; ++e) wt[k][e] = (float)(T)wt[k][e];
  }
}

struct DwLane {
  int cv, slot;
  bool live;
};
template <int V>
__device__ __forceinline__ DwLane dw_lane(const DwConvArgs& a) {
  DwLane l;
  l.slot = (int)threadIdx.x / a.CVt;
  l.cv = (int)blockIdx.y * a.CVt + (int)threadIdx.x % a.CVt;
  l.live = l.slot < a.PS && l.cv < a.C / V;
  return l;
}

// Sum K per-thread values over the pixel slots of the workgroup (slot order) and write them as rows
// row0 .. row0 + K / V - 1 of this workgroup's partial: part[(blockIdx.x * nrows + row) * C + c].
// red holds 256 * K values.  Threads that are not live pass zeros.
template <typename P, int K, int V>
__device__ __forceinline__ void dw_block_reduce(const DwConvArgs& a, const P (&v)[K], P* red, P* part, int nrows, int row0) {
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k * 256 + tid] = v[k];
  __syncthreads();
  const int CV = a.C / V;
  for (int idx = tid; idx < a.CVt * K; idx += 256) {
    const int k = idx / a.CVt, cvl = idx % a.CVt;
    P s = 0;
    for (int sl = 0; sl < a.PS; ++sl) s += red[k * 256 + sl * a.CVt + cvl];
    const int cv = (int)blockIdx.y * a.CVt + cvl;
    if (cv < CV)
      part[((long long)blockIdx.x * nrows + row0 + k / V) * a.C + cv * V + k % V] = s;
  }
  __syncthreads();
}

// run index -> (image, row, first column) over a grid of `rows` rows and rpr runs per row
__device__ __forceinline__ void dw_run(int run, int rpr, int rows, int& b, int& p, int& q0) {
  const int qr = run % rpr, rem = run / rpr;
  q0 = qr * kDwRun;
  p = rem % rows;
  b = rem / rows;
}

// ------------------------------------------------------------------------------------ forward
// TRAIN: t and the per-workgroup fp64 partials {sum t, sum t^2} [gridDim.x][2][C].
// !TRAIN: y = ((t - run_mean) rsqrt(run_var + eps)) gamma + beta, nothing else written.
template <typename T, int S, bool TRAIN>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(DwConvArgs a) {
  constexpr int V = DwVec<T>::N, R = kDwRun, NC = S * (R - 1) + 3;
  __shared__ double red[TRAIN ? 256 * 2 * V : 1];
  const DwLane ln = dw_lane<V>(a);
  double st[2 * V];
#pragma unroll
  for (int k = 0; k < 2 * V; ++k) st[k] = 0.0;
  if (ln.live) {
    const int c0 = ln.cv * V;
    float wt[9][V];
    dw_taps<T, V>(a.w, a.C, c0, wt);
    float mu[V], rs[V], ga[V], be[V];
    if constexpr (!TRAIN) {
      dw_ldf<V>(a.run_mean + c0, mu);
      dw_ldf<V>(a.run_var + c0, rs);
      dw_ldf<V>(a.gamma + c0, ga);
      dw_ldf<V>(a.beta + c0, be);
#pragma unroll
      for (int e = 0; e < V; ++e) rs[e] = 1.f / __builtin_sqrtf(rs[e] + a.eps);
    }
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
    T* __restrict__ out = reinterpret_cast<T*>(TRAIN ? a.t : a.y);
    for (int run = (int)blockIdx.x * a.PS + ln.slot; run < a.nruns; run += (int)gridDim.x * a.PS) {
      int b, p, q0;
      dw_run(run, a.rpr, a.Ho, b, p, q0);
      const int wbase = q0 * S - a.pl;
      float acc[R][V];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[r][e] = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int h = p * S + i - a.pt;
        const bool rowok = h >= 0 && h < a.H;
        const T* rowp = x + ((long long)b * a.H + h) * a.W * a.C + c0;
        typename DwVec<T>::raw xr[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int wc = wbase + c;
          xr[c] = dw_ld<T>(rowp + (long long)wc * a.C, rowok && wc >= 0 && wc < a.W);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[r][e] += (float)xr[S * r + j][e] * wt[3 * i + j][e];
      }
      T* op = out + (((long long)b * a.Ho + p) * a.Wo + q0) * a.C + c0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (q0 + r >= a.Wo) break;
        float tv[V];
#pragma unroll
        for (int e = 0; e < V; ++e) tv[e] = (float)(T)acc[r][e];
        if constexpr (TRAIN) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const double d = (double)tv[e];
            st[e] += d;
            st[V + e] += d * d;
          }
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) tv[e] = ((tv[e] - mu[e]) * rs[e]) * ga[e] + be[e];
        }
        dw_st<T>(op + (long long)r * a.C, tv);
      }
    }
  }
  if constexpr (TRAIN) dw_block_reduce<double, 2 * V, V>(a, st, red, reinterpret_cast<double*>(a.part), 2, 0);
}

// Sum the per-workgroup partial rows in a fixed order: kDwRedC columns x kDwRedS slices per
// workgroup, slice s takes partials s, s + kDwRedS, ... and the slices are added in slice order.
// STATS: part is [nparts][2][C] fp64 {sum t, sum t^2}: mean, rstd and the running statistics.
// else : part is [nparts][ncols] (P fp64 or fp32): column col goes to out0[col] (col < split) or
//        out1[col - split].
template <typename P, bool STATS>
__global__ __launch_bounds__(256) void dwconv_reduce_kernel(DwConvArgs a, int ncols, float* out0, float* out1, int split) {
  __shared__ double red[2][kDwRedS][kDwRedC + 1];
  constexpr int U = 4;   // partials in flight per thread: the pass is latency-bound
  const int cl = (int)threadIdx.x % kDwRedC, s = (int)threadIdx.x / kDwRedC;
  const int col = (int)blockIdx.x * kDwRedC + cl;
  const P* part = reinterpret_cast<const P*>(a.part);
  const long long stride = STATS ? 2LL * a.C : (long long)ncols;
  double s0 = 0.0, s1 = 0.0;
  if (col < ncols)
    for (int blk = s; blk < a.nparts; blk += U * kDwRedS) {
      P v0[U], v1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int bu = blk + u * kDwRedS;
        v0[u] = bu < a.nparts ? part[bu * stride + col] : (P)0;
        v1[u] = (STATS && bu < a.nparts) ? part[bu * stride + a.C + col] : (P)0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s0 += (double)v0[u];
        s1 += (double)v1[u];
      }
    }
  red[0][s][cl] = s0;
  red[1][s][cl] = s1;
  __syncthreads();
  if (s != 0 || col >= ncols) return;
  s0 = 0.0;
  s1 = 0.0;
#pragma unroll
  for (int k = 0; k < kDwRedS; ++k) {
    s0 += red[0][k][cl];
    s1 += red[1][k][cl];
  }
  if constexpr (STATS) {
    const double n = (double)a.npix;
    const double mu = s0 / n;
    double var = s1 / n - mu * mu;
    var = var > 0.0 ? var : 0.0;
    a.mean[col] = (float)mu;
    a.rstd[col] = (float)(1.0 / __builtin_sqrt(var + (double)a.eps));
    a.run_mean[col] = a.momentum * a.run_mean[col] + (1.f - a.momentum) * (float)mu;
    a.run_var[col] = a.momentum * a.run_var[col] + (1.f - a.momentum) * (float)var;
  } else {
    if (col < split) out0[col] = (float)s0;
    else out1[col - split] = (float)s0;
  }
}

// ------------------------------------------------------------------- the per-pixel passes
// y = ((t - mean) rstd) gamma + beta: a lane keeps its channel vector's constants and takes kDwPix
// pixels per trip (their loads in flight together)
template <typename T>
__global__ __launch_bounds__(256) void dwconv_norm_kernel(DwConvArgs a) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  const DwLane ln = dw_lane<V>(a);
  if (!ln.live) return;
  const int c0 = ln.cv * V;
  float mu[V], rs[V], ga[V], be[V];
  dw_ldf<V>(a.mean + c0, mu);
  dw_ldf<V>(a.rstd + c0, rs);
  dw_ldf<V>(a.gamma + c0, ga);
  dw_ldf<V>(a.beta + c0, be);
  const T* __restrict__ t = reinterpret_cast<const T*>(a.t) + c0;
  T* __restrict__ y = reinterpret_cast<T*>(a.y) + c0;
  const long long step = (long long)gridDim.x * a.PS;
  for (long long pix = (long long)blockIdx.x * a.PS + ln.slot; pix < a.npix; pix += U * step) {
    typename DwVec<T>::raw tr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) tr[u] = dw_ld<T>(t + (pix + u * step) * a.C, pix + u * step < a.npix);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (pix + u * step >= a.npix) break;
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = (((float)tr[u][e] - mu[e]) * rs[e]) * ga[e] + be[e];
      dw_st<T>(y + (pix + u * step) * a.C, v);
    }
  }
}

// per-workgroup fp64 partials {sum g, sum g xhat} [gridDim.x][2][C], xhat = (t - mean) rstd
template <typename T>
__global__ __launch_bounds__(256) void dwconv_bwd_sums_kernel(DwConvArgs a) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  __shared__ double red[256 * 2 * V];
  const DwLane ln = dw_lane<V>(a);
  double st[2 * V];
#pragma unroll
  for (int k = 0; k < 2 * V; ++k) st[k] = 0.0;
  if (ln.live) {
    const int c0 = ln.cv * V;
    float mu[V], rs[V];
    dw_ldf<V>(a.mean + c0, mu);
    dw_ldf<V>(a.rstd + c0, rs);
    const T* __restrict__ t = reinterpret_cast<const T*>(a.t) + c0;
    const T* __restrict__ g = reinterpret_cast<const T*>(a.dy) + c0;
    const long long step = (long long)gridDim.x * a.PS;
    for (long long pix = (long long)blockIdx.x * a.PS + ln.slot; pix < a.npix; pix += U * step) {
      typename DwVec<T>::raw tr[U], gr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = pix + u * step < a.npix;
        tr[u] = dw_ld<T>(t + (pix + u * step) * a.C, ok);
        gr[u] = dw_ld<T>(g + (pix + u * step) * a.C, ok);   // past the end: g = 0 adds nothing
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float gv = (float)gr[u][e];
          st[e] += (double)gv;
          st[V + e] += (double)(gv * (((float)tr[u][e] - mu[e]) * rs[e]));
        }
    }
  }
  dw_block_reduce<double, 2 * V, V>(a, st, red, reinterpret_cast<double*>(a.part), 2, 0);
}

// the constants of dt = A (g - KB - xhat KG): A = gamma rstd, KB = dbeta / N, KG = dgamma / N
template <int V>
struct DwDt {
  float mu[V], rs[V], A[V], KB[V], KG[V];
  __device__ __forceinline__ void load(const DwConvArgs& a, int c0) {
    dw_ldf<V>(a.mean + c0, mu);
    dw_ldf<V>(a.rstd + c0, rs);
    dw_ldf<V>(a.gamma + c0, A);
    dw_ldf<V>(a.dbeta + c0, KB);
    dw_ldf<V>(a.dgamma + c0, KG);
    const float invn = 1.f / (float)a.npix;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      A[e] *= rs[e];
      KB[e] *= invn;
      KG[e] *= invn;
    }
  }
  // ok == false (a position outside the output grid): zero
  template <typename RAW>
  __device__ __forceinline__ void at(const RAW& t, const RAW& g, bool ok, float (&d)[V]) const {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float xh = ((float)t[e] - mu[e]) * rs[e];
      d[e] = ok ? A[e] * ((float)g[e] - KB[e] - xh * KG[e]) : 0.f;
    }
  }
};

// ------------------------------------------------------------------------------- backward
// dx by gather: a lane takes kDwRun input pixels of one row and, for each of the (up to) three
// output rows that reach it, the NQ output columns that reach the run, of the dt the dw kernel left
// in the workspace (rounded to T there; recomputing it here from t and dy for every tap row took
// 83 us against 30 us here + 13 us more in the dw kernel, bf16 128 x 56 x 56 x 64 stride 1).  PL is the left padding (1 at stride 1; 0 or 1 at stride 2), which fixes which taps meet
// which columns at compile time.
template <typename T, int S, int PL>
__global__ __launch_bounds__(256) void dwconv_dx_kernel(DwConvArgs a) {
  constexpr int V = DwVec<T>::N, R = kDwRun, NQ = S == 1 ? R + 2 : R / 2 + 1;
  const DwLane ln = dw_lane<V>(a);
  if (!ln.live) return;
  const int c0 = ln.cv * V;
  float wt[9][V];
  dw_taps<T, V>(a.w, a.C, c0, wt);
  const T* __restrict__ dt = reinterpret_cast<const T*>(a.dt) + c0;
  T* __restrict__ dx = reinterpret_cast<T*>(a.dx) + c0;
  for (int run = (int)blockIdx.x * a.PS + ln.slot; run < a.nruns_in; run += (int)gridDim.x * a.PS) {
    int b, h, w0;
    dw_run(run, a.rpr_in, a.H, b, h, w0);
    const int qbase = S == 1 ? w0 - 1 : w0 / 2 - 1 + PL;
    float acc[R][V];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[r][e] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int hp = h + a.pt - i;
      if (hp < 0 || hp % S != 0 || hp / S >= a.Ho) continue;
      const long long row = ((long long)b * a.Ho + hp / S) * a.Wo;
      typename DwVec<T>::raw d[NQ];   // positions outside the output grid: zero
#pragma unroll
      for (int c = 0; c < NQ; ++c) {
        const int q = qbase + c;
        d[c] = dw_ld<T>(dt + (row + q) * a.C, q >= 0 && q < a.Wo);
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          constexpr int kOdd = S - 1;   // stride 2: only taps with q s + j = w + pl, i.e. r + PL - j even
          const int ev = r + PL - j;
          if ((ev & kOdd) != 0) continue;
          const int idx = S == 1 ? ev + 1 : ev / 2 + 1 - PL;
#pragma unroll
          for (int e = 0; e < V; ++e) acc[r][e] += wt[3 * i + j][e] * (float)d[idx][e];
        }
    }
    T* op = dx + (((long long)b * a.H + h) * a.W + w0) * a.C;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (w0 + r >= a.W) break;
      dw_st<T>(op + (long long)r * a.C, acc[r]);
    }
  }
}

// dw: the forward's walk with dt in the place of the taps; per-workgroup fp32 partials
// [gridDim.x][9][C], reduced over the slots one tap row at a time.  dt is computed here once per
// output position (fp32 for dw) and stored at T for the dx kernel, which runs after this one.
template <typename T, int S>
__global__ __launch_bounds__(256) void dwconv_dw_kernel(DwConvArgs a) {
  constexpr int V = DwVec<T>::N, R = kDwRun, NC = S * (R - 1) + 3;
  __shared__ float red[256 * 3 * V];
  const DwLane ln = dw_lane<V>(a);
  float acc[3][3 * V];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3 * V; ++k) acc[i][k] = 0.f;
  if (ln.live) {
    const int c0 = ln.cv * V;
    DwDt<V> k;
    k.load(a, c0);
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x);
    const T* __restrict__ t = reinterpret_cast<const T*>(a.t) + c0;
    const T* __restrict__ g = reinterpret_cast<const T*>(a.dy) + c0;
    T* __restrict__ dt = reinterpret_cast<T*>(a.dt) + c0;
    for (int run = (int)blockIdx.x * a.PS + ln.slot; run < a.nruns; run += (int)gridDim.x * a.PS) {
      int b, p, q0;
      dw_run(run, a.rpr, a.Ho, b, p, q0);
      const long long o0 = (((long long)b * a.Ho + p) * a.Wo + q0) * a.C;
      float d[R][V];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool ok = q0 + r < a.Wo;
        k.at(dw_ld<T>(t + o0 + (long long)r * a.C, ok), dw_ld<T>(g + o0 + (long long)r * a.C, ok), ok, d[r]);
        if (ok) dw_st<T>(dt + o0 + (long long)r * a.C, d[r]);
      }
      const int wbase = q0 * S - a.pl;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int h = p * S + i - a.pt;
        const bool rowok = h >= 0 && h < a.H;
        const T* rowp = x + ((long long)b * a.H + h) * a.W * a.C + c0;
        typename DwVec<T>::raw xr[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int wc = wbase + c;
          xr[c] = dw_ld<T>(rowp + (long long)wc * a.C, rowok && wc >= 0 && wc < a.W);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[i][j * V + e] += (float)xr[S * r + j][e] * d[r][e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    dw_block_reduce<float, 3 * V, V>(a, acc[i], red, reinterpret_cast<float*>(a.part), 9, 3 * i);
}

}  // namespace sae

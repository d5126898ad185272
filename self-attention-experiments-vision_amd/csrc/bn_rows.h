// bn_rows.h -- BatchNorm over token rows followed by the tanh-GELU, forward and backward: the
// operation the CeiT locally-enhanced feed-forward applies three times
// (models/layers/feedforwards/leff.py:39-59), with the class token split off in front of the first
// and re-attached behind the last.
//
// x [B][L + x_lead][C] in the compute dtype T (bf16 or fp32); x_lead (0 or 1) leading rows per sample
// are skipped, N = B L rows take part.  y [B][L + y_lead][C]; with y_lead = 1 row 0 of every sample
// of y is a copy of `lead` (one row of C per sample, sample pitch lead_pitch elements).
//     training:   mu, var = biased batch statistics per channel (fp64 sums of x and x^2),
//                 r = rsqrt(var + eps), z = T( ((x - mu) r) gamma + beta ), y = T( gelu(z) ),
//                 run_mean = m run_mean + (1 - m) mu, run_var = m run_var + (1 - m) var
//     evaluation: the same formula with run_mean / run_var, one kernel, buffers untouched
//     backward:   z recomputed (the same expression, the same rounding), dz = g gelu'(z) with g = dy
//                 in y's layout, dbeta = sum dz, dgamma = sum dz xhat,
//                 dx = T( gamma r (dz - dbeta / N - xhat dgamma / N) ) in x's layout, its skipped
//                 lead rows written as zeros (the gradient of `lead` is row 0 of dy: a view)
// z is used and never stored: the forward reads x twice and writes y once, the backward reads x and
// dy twice and writes dx once; mean and rstd (fp32 [C]) are all that is saved.  gelu / gelu' are
// gelu_f / dgelu_f of gelu.h, the functions of the FF GEMM epilogues.
//
// Layout and reductions are those of dwconv.h, whose lane map (dw_lane), workgroup reduction
// (dw_block_reduce), partial-row reduce kernels (dwconv_reduce_kernel) and argument block are used
// as they are: the 16-byte channel vector innermost on the lanes, a thread = one channel vector x one
// row slot with its BatchNorm constants in registers, kDwPix rows in flight per thread, parallelism
// over rows (C = 192 fills the chip); per-thread fp64 partials summed through LDS in slot order, one
// partial row per workgroup, summed over the workgroups in index order.  No floating-point atomics:
// two calls on the same inputs agree bit for bit.  Of DwConvArgs these kernels read x, y, dy, dx,
// gamma, beta, run_mean, run_var, mean, rstd, dgamma, dbeta, part, C, CVt, PS, npix (= N), eps.
#pragma once
#include "dwconv.h"
#include "gelu.h"

namespace sae {

struct BnRows {
  const void* lead;       // [B] rows of C elements (y_lead == 1)
  long long lead_pitch;   // elements between the lead rows of consecutive samples
  int L, x_lead, y_lead;
  int rows_x, rows_y;     // B (L + x_lead), B (L + y_lead)
  FDiv dL, dLx, dLy;      // division by L, L + x_lead, L + y_lead
};

// participating row n = b L + l -> its row in a layout with `lead` leading rows per sample
__device__ __forceinline__ long long bn_row(const BnRows& r, long long n, int lead) {
  return n + (long long)(r.dL.div((int)n) + 1) * lead;
}

// the BatchNorm constants of a thread's channel vector and z, xhat of one element
template <typename T, int V>
struct BnConst {
  float mu[V], rs[V], ga[V], be[V];
  // batch: the saved mean / rstd; else the running statistics
  __device__ __forceinline__ void load(const DwConvArgs& a, int c0, bool batch) {
    dw_ldf<V>((batch ? a.mean : a.run_mean) + c0, mu);
    dw_ldf<V>((batch ? a.rstd : a.run_var) + c0, rs);
    dw_ldf<V>(a.gamma + c0, ga);
    dw_ldf<V>(a.beta + c0, be);
    if (!batch) {
#pragma unroll
      for (int e = 0; e < V; ++e) rs[e] = 1.f / __builtin_sqrtf(rs[e] + a.eps);
    }
  }
  __device__ __forceinline__ float xhat(float x, int e) const { return (x - mu[e]) * rs[e]; }
  // one expression for the forward and the backward's recomputation: an explicit fma, so that the
  // two kernels cannot be contracted differently
  __device__ __forceinline__ float z(float x, int e) const {
    return (float)(T)__builtin_fmaf(xhat(x, e), ga[e], be[e]);
  }
};

// dz = g gelu'(z), rounded to fp32 before anything uses it.  The empty asm keeps the product out of
// an fma with the subtraction that follows in the dx kernel: contracted, dz - dbeta / N would see the
// unrounded product there and the rounded one in dbeta, and at N = 1 (rstd = rsqrt(eps)) that
// residue, times gamma rstd, is a dx of 4e-5 where the exact answer is 0.
__device__ __forceinline__ float bn_dz(float g, float z) {
  float dz = g * dgelu_f(z);
  asm("" : "+v"(dz));
  return dz;
}

// ------------------------------------------------------------------------------------ forward
// per-workgroup fp64 partials {sum x, sum x^2} [gridDim.x][2][C] over the N participating rows
template <typename T>
__global__ __launch_bounds__(256) void bn_rows_stats_kernel(DwConvArgs a, BnRows r) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  __shared__ double red[256 * 2 * V];
  const DwLane ln = dw_lane<V>(a);
  double st[2 * V];
#pragma unroll
  for (int k = 0; k < 2 * V; ++k) st[k] = 0.0;
  if (ln.live) {
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + ln.cv * V;
    const long long step = (long long)gridDim.x * a.PS;
    for (long long n = (long long)blockIdx.x * a.PS + ln.slot; n < a.npix; n += U * step) {
      typename DwVec<T>::raw xr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long nu = n + u * step;
        const bool ok = nu < a.npix;
        xr[u] = dw_ld<T>(x + (ok ? bn_row(r, nu, r.x_lead) : 0) * a.C, ok);   // past the end: x = 0 adds nothing
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double d = (double)(float)xr[u][e];
          st[e] += d;
          st[V + e] += d * d;
        }
    }
  }
  dw_block_reduce<double, 2 * V, V>(a, st, red, reinterpret_cast<double*>(a.part), 2, 0);
}

// y over the rows of y's layout: a lead row is copied from `lead`, every other row is
// T(gelu(z)) of its row of x.  TRAIN: the batch statistics of mean / rstd; else the running ones.
template <typename T, bool TRAIN>
__global__ __launch_bounds__(256) void bn_rows_apply_kernel(DwConvArgs a, BnRows r) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  const DwLane ln = dw_lane<V>(a);
  if (!ln.live) return;
  const int c0 = ln.cv * V;
  BnConst<T, V> k;
  k.load(a, c0, TRAIN);
  const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + c0;
  const T* __restrict__ lead = reinterpret_cast<const T*>(r.lead) + c0;
  T* __restrict__ y = reinterpret_cast<T*>(a.y) + c0;
  const int Ly = r.L + r.y_lead;
  const long long step = (long long)gridDim.x * a.PS;
  for (long long ry = (long long)blockIdx.x * a.PS + ln.slot; ry < r.rows_y; ry += U * step) {
    typename DwVec<T>::raw xr[U];
    bool copy[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long ru = ry + u * step;
      const bool ok = ru < r.rows_y;
      const int b = ok ? r.dLy.div((int)ru) : 0;
      copy[u] = ok && (int)ru - b * Ly < r.y_lead;
      const long long n = ru - (long long)(b + 1) * r.y_lead;   // (a participating row when !copy)
      const T* src = copy[u] ? lead + (long long)b * r.lead_pitch : x + (n + (long long)(b + 1) * r.x_lead) * a.C;
      xr[u] = dw_ld<T>(src, ok);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long ru = ry + u * step;
      if (ru >= r.rows_y) break;
      if (copy[u]) {
        *reinterpret_cast<typename DwVec<T>::raw*>(y + ru * a.C) = xr[u];
        continue;
      }
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = gelu_f(k.z((float)xr[u][e], e));
      dw_st<T>(y + ru * a.C, v);
    }
  }
}

// ----------------------------------------------------------------------------------- backward
// per-workgroup fp64 partials {sum dz, sum dz xhat} [gridDim.x][2][C], dz = dy gelu'(z)
template <typename T>
__global__ __launch_bounds__(256) void bn_rows_bwd_sums_kernel(DwConvArgs a, BnRows r) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  __shared__ double red[256 * 2 * V];
  const DwLane ln = dw_lane<V>(a);
  double st[2 * V];
#pragma unroll
  for (int k = 0; k < 2 * V; ++k) st[k] = 0.0;
  if (ln.live) {
    const int c0 = ln.cv * V;
    BnConst<T, V> k;
    k.load(a, c0, true);
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + c0;
    const T* __restrict__ g = reinterpret_cast<const T*>(a.dy) + c0;
    const long long step = (long long)gridDim.x * a.PS;
    for (long long n = (long long)blockIdx.x * a.PS + ln.slot; n < a.npix; n += U * step) {
      typename DwVec<T>::raw xr[U], gr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long nu = n + u * step;
        const bool ok = nu < a.npix;
        const int b1 = ok ? r.dL.div((int)nu) + 1 : 0;
        xr[u] = dw_ld<T>(x + (ok ? nu + (long long)b1 * r.x_lead : 0) * a.C, ok);
        gr[u] = dw_ld<T>(g + (ok ? nu + (long long)b1 * r.y_lead : 0) * a.C, ok);   // past the end: g = 0 adds nothing
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xv = (float)xr[u][e];
          const float dz = bn_dz((float)gr[u][e], k.z(xv, e));
          st[e] += (double)dz;
          st[V + e] += (double)(dz * k.xhat(xv, e));
        }
    }
  }
  dw_block_reduce<double, 2 * V, V>(a, st, red, reinterpret_cast<double*>(a.part), 2, 0);
}

// dx over the rows of x's layout (the constants of DwDt: A = gamma rstd, KB = dbeta / N,
// KG = dgamma / N); a skipped lead row is written as zeros
template <typename T>
__global__ __launch_bounds__(256) void bn_rows_dx_kernel(DwConvArgs a, BnRows r) {
  constexpr int V = DwVec<T>::N, U = kDwPix;
  const DwLane ln = dw_lane<V>(a);
  if (!ln.live) return;
  const int c0 = ln.cv * V;
  BnConst<T, V> k;
  k.load(a, c0, true);
  DwDt<V> d;
  d.load(a, c0);
  const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + c0;
  const T* __restrict__ g = reinterpret_cast<const T*>(a.dy) + c0;
  T* __restrict__ dx = reinterpret_cast<T*>(a.dx) + c0;
  const int Lx = r.L + r.x_lead;
  const long long step = (long long)gridDim.x * a.PS;
  for (long long rx = (long long)blockIdx.x * a.PS + ln.slot; rx < r.rows_x; rx += U * step) {
    typename DwVec<T>::raw xr[U], gr[U];
    bool part[U];   // the row takes part (it is no skipped lead row)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long ru = rx + u * step;
      const bool ok = ru < r.rows_x;
      const int b = ok ? r.dLx.div((int)ru) : 0;
      part[u] = ok && (int)ru - b * Lx >= r.x_lead;
      const long long n = ru - (long long)(b + 1) * r.x_lead;
      xr[u] = dw_ld<T>(x + (part[u] ? ru : 0) * a.C, part[u]);
      gr[u] = dw_ld<T>(g + (part[u] ? n + (long long)(b + 1) * r.y_lead : 0) * a.C, part[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long ru = rx + u * step;
      if (ru >= r.rows_x) break;
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xv = (float)xr[u][e];
        const float dz = bn_dz((float)gr[u][e], k.z(xv, e));
        v[e] = part[u] ? d.A[e] * (dz - d.KB[e] - k.xhat(xv, e) * d.KG[e]) : 0.f;
      }
      dw_st<T>(dx + ru * a.C, v);
    }
  }
}

}  // namespace sae

// convtok.h -- the CvT convolutional token embedding (models/cvt.py:19-35): a dense k x k
// convolution with stride s < k and Flax SAME padding, as a window matrix written once and the
// project's GEMMs on it (the route measured as the faster one for the patch embedding,
// patch_gather_hwcn_kernel in patch.h: write the operand, then run the LDS-DMA kernels).
//
//   x [B][H][W][C] (NHWC), Ho = ceil(H / s), Wo = ceil(W / s), M = B Ho Wo, K = k k C,
//   Kp = K rounded up to a multiple of 8, pads: total = max((Ho - 1) s + k - H, 0), pt = total / 2
//   gather :  P[m][(ky k + kx) C + c] = x[b][oy s - pt + ky][ox s - pl + kx][c]      m = (b, oy, ox)
//             zero for taps outside the image and for the columns K .. Kp
//   scatter:  dX[b][iy][ix][c] = sum_{ky, kx} dP[m(b, oy, ox)][(ky k + kx) C + c]
//             over the windows with oy s + ky = iy + pt, 0 <= oy < Ho (and the same in x)
//
// The column order is the Flax kernel [kh, kw, in, out] viewed as [k k C, out], so the convolution
// is P W, its weight gradient P^T dY and its input gradient the scatter of dY W^T.
//
// One thread writes one 16-byte chunk of its output (8 bf16 or 4 fp32).  VEC (C a multiple of the
// chunk): a chunk lies inside one tap, one 16-byte load (two for fp32 rounded to bf16) per 16-byte
// store, and consecutive lanes read consecutive chunks of one image row.  !VEC (the first stage,
// C = 3): element loads.  The scatter is a gather over the at most ceil(k / s)^2 windows that
// cover a pixel, summed in fp32 with ky ascending, then kx ascending: no atomics, the same bits on
// every run.  Every index fits 32 bits: the host refuses extents whose element offsets do not.
#pragma once
#include <type_traits>

#include "common.h"

namespace sae {

struct ConvTokGeom {
  int B, H, W, C, k, s, Ho, Wo, pt, pl;
  int K, Kp, M;           // k k C, K rounded up to 8, B Ho Wo
  int nch, total;         // gather: 16-byte chunks per row of P, threads
  int cch, total_s;       // scatter: channel chunks per pixel, threads
  FDiv dnch, dHoWo, dWo, dC, dk;   // gather
  FDiv dcch, dHW, dW, ds;          // scatter
};

template <typename T> struct CtVec;
template <> struct CtVec<__bf16> {
  static constexpr int N = 8;
  using raw = bf16x8;
};
template <> struct CtVec<float> {
  static constexpr int N = 4;
  using raw = f32x4;
};

// N consecutive elements of x as TO (fp32 -> bf16: rounded to nearest even as they are staged)
template <typename TI, typename TO>
__device__ __forceinline__ typename CtVec<TO>::raw ct_load(const TI* p) {
  if constexpr (std::is_same<TI, TO>::value) {
    return *reinterpret_cast<const typename CtVec<TO>::raw*>(p);
  } else {
    const f32x4 u = reinterpret_cast<const f32x4*>(p)[0], v = reinterpret_cast<const f32x4*>(p)[1];
    return bf16x8{(__bf16)u[0], (__bf16)u[1], (__bf16)u[2], (__bf16)u[3],
                  (__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  }
}

// ---- the window matrix.  Thread (m, chunk): columns col0 .. col0 + N - 1 of row m.
template <typename TI, typename TO, bool VEC>
__global__ __launch_bounds__(256) void conv_window_gather_kernel(ConvTokGeom g, const TI* __restrict__ x,
                                                                 TO* __restrict__ P) {
  constexpr int N = CtVec<TO>::N;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)g.total) return;
  const int m = g.dnch.div((int)idx), ch = (int)idx - m * g.nch;
  const int b = g.dHoWo.div(m), p = m - b * (g.Ho * g.Wo);
  const int oy = g.dWo.div(p), ox = p - oy * g.Wo;
  const int iy0 = oy * g.s - g.pt, ix0 = ox * g.s - g.pl;
  const int col0 = ch * N;
  typename CtVec<TO>::raw out = {};
  if constexpr (VEC) {
    if (col0 < g.K) {   // (K is a multiple of N here: a chunk is inside one tap or all padding)
      const int tap = g.dC.div(col0), c0 = col0 - tap * g.C;
      const int ky = g.dk.div(tap), kx = tap - ky * g.k;
      const int iy = iy0 + ky, ix = ix0 + kx;
      if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
        out = ct_load<TI, TO>(x + (((unsigned)(b * g.H + iy) * g.W + ix) * g.C + c0));
    }
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int col = col0 + j;
      if (col >= g.K) break;
      const int tap = g.dC.div(col), c = col - tap * g.C;
      const int ky = g.dk.div(tap), kx = tap - ky * g.k;
      const int iy = iy0 + ky, ix = ix0 + kx;
      if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) out[j] = (TO)x[((unsigned)(b * g.H + iy) * g.W + ix) * g.C + c];
    }
  }
  *reinterpret_cast<typename CtVec<TO>::raw*>(P + ((unsigned)m * g.Kp + col0)) = out;
}

// ---- the input gradient.  Thread (pixel, channel chunk): channels c0 .. c0 + N - 1 of one pixel.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void conv_window_scatter_kernel(ConvTokGeom g, const T* __restrict__ dP,
                                                                  T* __restrict__ dX) {
  constexpr int N = CtVec<T>::N;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)g.total_s) return;
  const int pix = g.dcch.div((int)idx), c0 = ((int)idx - pix * g.cch) * N;
  const int b = g.dHW.div(pix), r = pix - b * (g.H * g.W);
  const int iy = g.dW.div(r), ix = r - iy * g.W;
  // window oy with tap ky covers the row when oy s + ky = iy + pt: the smallest ky is (iy + pt) % s
  const int ty = iy + g.pt, tx = ix + g.pl;
  const int qy = g.ds.div(ty), ky0 = ty - qy * g.s;
  const int qx = g.ds.div(tx), kx0 = tx - qx * g.s;
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  for (int ky = ky0, oy = qy; ky < g.k && oy >= 0; ky += g.s, --oy) {
    if (oy >= g.Ho) continue;
    for (int kx = kx0, ox = qx; kx < g.k && ox >= 0; kx += g.s, --ox) {
      if (ox >= g.Wo) continue;
      const T* src = dP + ((unsigned)((b * g.Ho + oy) * g.Wo + ox) * g.Kp + (ky * g.k + kx) * g.C + c0);
      if constexpr (VEC) {
        const typename CtVec<T>::raw v = *reinterpret_cast<const typename CtVec<T>::raw*>(src);
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] += (float)v[e];
      } else {
#pragma unroll
        for (int e = 0; e < N; ++e)
          if (c0 + e < g.C) acc[e] += (float)src[e];
      }
    }
  }
  T* dst = dX + ((unsigned)pix * g.C + c0);
  if constexpr (VEC) {
    typename CtVec<T>::raw o;
#pragma unroll
    for (int e = 0; e < N; ++e) o[e] = (T)acc[e];
    *reinterpret_cast<typename CtVec<T>::raw*>(dst) = o;
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (c0 + e < g.C) dst[e] = (T)acc[e];
  }
}

}  // namespace sae

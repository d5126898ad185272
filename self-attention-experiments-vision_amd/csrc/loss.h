// loss.h -- the training step's label-smoothed softmax cross entropy, forward and backward (the
// §8f "DP train-step harness" row).
//
// Reference: train.py:77-90 -- y = optax.smooth_labels(one_hot(labels), alpha) = (1 - alpha) onehot
// + alpha / K, loss = mean_r optax.softmax_cross_entropy(logits_r, y_r) = mean_r -sum_c y_rc
// log_softmax(logits_r)_c, which per row is
//     lse_r - (1 - alpha) x[r, label_r] - (alpha / K) sum_c x[r, c]
// and whose gradient is  dlogits[r, c] = (g / R) (exp(x[r, c] - lse_r) - (1 - alpha) [c == label_r] - alpha / K).
// Replaces ~25 small framework launches (upcast, log-softmax, nll, smoothing sums, their
// backward) with three: the forward takes one workgroup per row (fp32 max / sum-exp / sum) and
// writes lse_r and the row's loss, one workgroup sums the row losses in a fixed order
// (deterministic), and the backward writes dlogits in the logits' dtype (bf16 or fp32), one
// workgroup per row.
#pragma once
#include "common.h"

namespace sae {

template <typename T> __device__ __forceinline__ float ce_ld(const T* p, long long i) { return (float)p[i]; }

__device__ __forceinline__ float ce_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float ce_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// forward, one 256-thread workgroup per row: lse_r and the row's smoothed loss
template <typename T>
__global__ __launch_bounds__(256) void smoothed_ce_fwd_kernel(const T* __restrict__ x, long long ld,
                                                              const int64_t* __restrict__ labels, int K, float alpha,
                                                              float* __restrict__ lse, float* __restrict__ row_loss) {
  __shared__ float red[2][4];
  const int r = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T* xr = x + (long long)r * ld;
  float m = -INFINITY, sx = 0.f;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float v = ce_ld(xr, c);
    m = fmaxf(m, v);
    sx += v;
  }
  m = ce_wave_max(m);
  sx = ce_wave_sum(sx);
  if (lane == 0) {
    red[0][w] = m;
    red[1][w] = sx;
  }
  __syncthreads();
  m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  sx = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  __syncthreads();
  float se = 0.f;
  for (int c = threadIdx.x; c < K; c += 256) se += __expf(ce_ld(xr, c) - m);
  se = ce_wave_sum(se);
  if (lane == 0) red[0][w] = se;
  __syncthreads();
  if (threadIdx.x == 0) {
    se = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float l = m + __logf(se);
    const int64_t y = labels[r];
    const float xy = (y >= 0 && y < K) ? ce_ld(xr, (long long)y) : 0.f;
    lse[r] = l;
    row_loss[r] = l - (1.f - alpha) * xy - (alpha / (float)K) * sx;
  }
}

// the mean over rows, summed in row order by one workgroup (deterministic)
__global__ __launch_bounds__(256) void smoothed_ce_mean_kernel(const float* __restrict__ row_loss, int R,
                                                               float* __restrict__ loss) {
  __shared__ float part[256];
  // thread t sums the contiguous rows [t * per, (t + 1) * per), then thread 0 adds the 256 parts in order
  const int per = (R + 255) / 256;
  float s = 0.f;
  for (int r = threadIdx.x * per; r < min(R, (threadIdx.x + 1) * per); ++r) s += row_loss[r];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < 256; ++i) t += part[i];
    *loss = t / (float)R;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void smoothed_ce_bwd_kernel(const T* __restrict__ x, long long ld,
                                                              const int64_t* __restrict__ labels, int R, int K,
                                                              float alpha, const float* __restrict__ lse,
                                                              const float* __restrict__ gloss, T* __restrict__ dx,
                                                              long long ldd) {
  const int r = blockIdx.x;
  const float g = *gloss / (float)R, l = lse[r], off = alpha / (float)K;
  const int64_t y = labels[r];
  const T* xr = x + (long long)r * ld;
  T* dr = dx + (long long)r * ldd;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float p = __expf(ce_ld(xr, c) - l);
    dr[c] = (T)(g * (p - (c == y ? 1.f - alpha : 0.f) - off));
  }
}

// ------------------------------------------------------------------ mixup / cutmix targets, top-k
// Reference: train.py:83-90 with the default augmentation -- the target is rho onehot(y0) +
// (1 - rho) onehot(y1) before optax.smooth_labels, so per row
//     lse_r - (1 - alpha) (rho x[r, y0] + (1 - rho) x[r, y1]) - (alpha / K) sum_c x[r, c]
// and dlogits[r, c] = (g / R) (softmax - (1 - alpha) (rho [c == y0] + (1 - rho) [c == y1]) - alpha / K).
// mix == nullptr (rho = 1, no second label) and rho == 1 repeat the arithmetic of the kernels above
// bit for bit: rho x0 + 0 x1 is x0 and (1 - alpha) 1 is 1 - alpha.
//
// The same forward also ranks the first label as utils.topk_correct (train.py:98-99) does: rank_r =
// the number of classes a stable ascending argsort of the row places above y0, counted in the pass
// that re-reads the row for sum-exp.  The order is the sort's total order on the bits (the library
// is built with -fno-honor-nans, so no float comparison sees a NaN): NaN above everything, -0 == +0,
// equal values ordered by class index.

// a key whose unsigned order is the sort's order of the values
__device__ __forceinline__ unsigned ce_sort_key(float v) {
  unsigned u = __float_as_uint(v);
  const unsigned mag = u & 0x7fffffffu;
  if (mag > 0x7f800000u) return 0xffffffffu;   // NaN (either sign): last, all equal
  if (mag == 0u) u = 0u;                       // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int ce_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// forward, one 256-thread workgroup per row: lse_r, the row's loss and (rank != nullptr) the label's rank
template <typename T>
__global__ __launch_bounds__(256) void mixed_ce_fwd_kernel(const T* __restrict__ x, long long ld,
                                                           const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ mix,
                                                           const float* __restrict__ ratio, int K, float alpha,
                                                           float* __restrict__ lse, float* __restrict__ row_loss,
                                                           int* __restrict__ rank) {
  __shared__ float red[2][4];
  __shared__ int redn[4];
  const int r = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T* xr = x + (long long)r * ld;
  float m = -INFINITY, sx = 0.f;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float v = ce_ld(xr, c);
    m = fmaxf(m, v);
    sx += v;
  }
  m = ce_wave_max(m);
  sx = ce_wave_sum(sx);
  if (lane == 0) {
    red[0][w] = m;
    red[1][w] = sx;
  }
  __syncthreads();
  m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  sx = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  __syncthreads();
  const int64_t y = labels[r];
  const bool y_ok = y >= 0 && y < K;
  const unsigned ky = y_ok ? ce_sort_key(ce_ld(xr, (long long)y)) : 0u;
  float se = 0.f;
  int above = 0;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float v = ce_ld(xr, c);
    se += __expf(v - m);
    const unsigned kc = ce_sort_key(v);
    above += (kc > ky || (kc == ky && c > (int)y)) ? 1 : 0;
  }
  se = ce_wave_sum(se);
  above = ce_wave_sum_int(above);
  if (lane == 0) {
    red[0][w] = se;
    redn[w] = above;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    se = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float l = m + __logf(se);
    float xy = y_ok ? ce_ld(xr, (long long)y) : 0.f;
    if (mix) {
      const int64_t y1 = mix[r];
      const float rho = ratio[r];
      const float x1 = (y1 >= 0 && y1 < K) ? ce_ld(xr, (long long)y1) : 0.f;
      xy = rho * xy + (1.f - rho) * x1;
    }
    lse[r] = l;
    row_loss[r] = l - (1.f - alpha) * xy - (alpha / (float)K) * sx;
    if (rank) rank[r] = y_ok ? ((redn[0] + redn[1]) + redn[2]) + redn[3] : K;
  }
}

// the mean over rows in the order of smoothed_ce_mean_kernel, and (rank != nullptr) the fractions of
// rows whose label ranks in the top 1 / top 5: integer counts, so their order does not matter
__global__ __launch_bounds__(256) void mixed_ce_mean_kernel(const float* __restrict__ row_loss,
                                                            const int* __restrict__ rank, int R,
                                                            float* __restrict__ loss, float* __restrict__ top) {
  __shared__ float part[256];
  __shared__ int hit[2][256];
  const int per = (R + 255) / 256;
  float s = 0.f;
  int h1 = 0, h5 = 0;
  for (int r = threadIdx.x * per; r < min(R, (threadIdx.x + 1) * per); ++r) {
    s += row_loss[r];
    if (rank) {
      h1 += rank[r] < 1;
      h5 += rank[r] < 5;
    }
  }
  part[threadIdx.x] = s;
  hit[0][threadIdx.x] = h1;
  hit[1][threadIdx.x] = h5;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    int t1 = 0, t5 = 0;
    for (int i = 0; i < 256; ++i) {
      t += part[i];
      t1 += hit[0][i];
      t5 += hit[1][i];
    }
    *loss = t / (float)R;
    if (rank) {
      top[0] = (float)t1 / (float)R;
      top[1] = (float)t5 / (float)R;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mixed_ce_bwd_kernel(const T* __restrict__ x, long long ld,
                                                           const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ mix,
                                                           const float* __restrict__ ratio, int R, int K,
                                                           float alpha, const float* __restrict__ lse,
                                                           const float* __restrict__ gloss, T* __restrict__ dx,
                                                           long long ldd) {
  const int r = blockIdx.x;
  const float g = *gloss / (float)R, l = lse[r], off = alpha / (float)K;
  const int64_t y = labels[r], y1 = mix ? mix[r] : -1;
  const float rho = mix ? ratio[r] : 1.f;
  const T* xr = x + (long long)r * ld;
  T* dr = dx + (long long)r * ldd;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float p = __expf(ce_ld(xr, c) - l);
    const float t = (1.f - alpha) * ((c == y ? rho : 0.f) + (c == y1 ? 1.f - rho : 0.f));
    dr[c] = (T)(g * (p - t - off));
  }
}

// The evaluation accumulator {double loss_sum; int64 top1, top5, samples}: one workgroup adds a
// batch's row losses (in double, in row order: thread 0 alone) and its hit counts.  Stream-ordered
// read-modify-write by one thread: replays of a captured graph keep accumulating.
// Cost: the ordered sum is one thread's chain, about 10 ns per row once the rows come from LDS --
// measured per call, back-to-back launches on one MI355X: 7.6 us at R = 128, 16 us at 1024, 46 us at
// 4096, 166 us at SAE_CE_MAX_ROWS (reading global memory directly it was 11 / 45 / 163 / 635 us).
// Evaluation batches are a few hundred rows per GPU, beside a forward of milliseconds.
struct CeAccum {
  double loss_sum;
  long long top1, top5, samples;
};
constexpr int kCeStage = 1024;   // row losses staged in LDS per trip

__global__ __launch_bounds__(256) void ce_accumulate_kernel(const float* __restrict__ row_loss,
                                                            const int* __restrict__ rank, int R,
                                                            CeAccum* __restrict__ acc) {
  __shared__ int hit[2][256];
  int h1 = 0, h5 = 0;
  for (int r = threadIdx.x; r < R; r += 256) {
    h1 += rank[r] < 1;
    h5 += rank[r] < 5;
  }
  hit[0][threadIdx.x] = h1;
  hit[1][threadIdx.x] = h5;
  // the row losses pass through LDS, kCeStage at a time (coalesced loads by the whole workgroup),
  // so that thread 0's ordered chain of double adds reads LDS, not global memory; R is uniform,
  // so every thread makes the same trips through the barriers
  __shared__ float stage[kCeStage];
  double s = 0.0;
  if (threadIdx.x == 0) s = acc->loss_sum;
  for (int r0 = 0; r0 < R; r0 += kCeStage) {
    const int n = min(kCeStage, R - r0);
    for (int i = threadIdx.x; i < n; i += 256) stage[i] = row_loss[r0 + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) s += (double)stage[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    long long t1 = 0, t5 = 0;
    for (int i = 0; i < 256; ++i) {
      t1 += hit[0][i];
      t5 += hit[1][i];
    }
    acc->loss_sum = s;
    acc->top1 += t1;
    acc->top5 += t5;
    acc->samples += R;
  }
}

}  // namespace sae

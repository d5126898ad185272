// loss.h -- the training step's softmax cross entropy, forward and backward (the §8f "DP train-step
// harness" row): one kernel family for the label-smoothed loss, its mixup / cutmix form and the
// top-k ranks, and the evaluation accumulator.
//
// Reference: train.py:77-90 -- the target is rho onehot(y0) + (1 - rho) onehot(y1) (the default
// augmentation's mixup / cutmix; one label per row is rho = 1), y = optax.smooth_labels(target, alpha)
// = (1 - alpha) target + alpha / K, loss = mean_r optax.softmax_cross_entropy(logits_r, y_r) = mean_r
// -sum_c y_rc log_softmax(logits_r)_c, which per row is
//     lse_r - (1 - alpha) (rho x[r, y0] + (1 - rho) x[r, y1]) - (alpha / K) sum_c x[r, c]
// and whose gradient is
//     dlogits[r, c] = (g / R) (exp(x[r, c] - lse_r) - (1 - alpha) (rho [c == y0] + (1 - rho) [c == y1]) - alpha / K).
// The special case: mix == nullptr is one label per row (rho = 1, no y1), the plain smoothed loss
//     lse_r - (1 - alpha) x[r, y0] - (alpha / K) sum_c x[r, c];
// rho == 1 with any partner gives the same bits (rho x0 + 0 x1 is x0 and (1 - alpha) (1 + 0) is 1 - alpha).
// Replaces ~25 small framework launches (upcast, log-softmax, nll, smoothing sums, their
// backward) with three: the forward takes one workgroup per row (fp32 max / sum-exp / sum) and
// writes lse_r and the row's loss, one workgroup sums the row losses in a fixed order
// (deterministic), and the backward writes dlogits in the logits' dtype (bf16 or fp32), one
// workgroup per row.
//
// RANK: the same forward also ranks the first label as utils.topk_correct (train.py:98-99) does:
// rank_r = the number of classes a stable ascending argsort of the row places above y0, counted in
// the pass that re-reads the row for sum-exp.  The order is the sort's total order on the bits (the
// library is built with -fno-honor-nans, so no float comparison sees a NaN): NaN above everything,
// -0 == +0, equal values ordered by class index.  RANK == false compiles none of it.
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

// forward, one 256-thread workgroup per row: lse_r, the row's loss and (RANK) the first label's rank.
// mix (with ratio) is read by thread 0 alone, after the reductions.
template <typename T, bool RANK>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const T* __restrict__ x, long long ld,
                                                     const int64_t* __restrict__ labels,
                                                     const int64_t* __restrict__ mix, const float* __restrict__ ratio,
                                                     int K, float alpha, float* __restrict__ lse,
                                                     float* __restrict__ row_loss, int* __restrict__ rank) {
  __shared__ float red[2][4];
  __shared__ int redn[4];   // (RANK only)
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
  if constexpr (RANK) {
    const int64_t y = labels[r];
    const unsigned ky = (y >= 0 && y < K) ? ce_sort_key(ce_ld(xr, (long long)y)) : 0u;
    int above = 0;
    for (int c = threadIdx.x; c < K; c += 256) {
      const float v = ce_ld(xr, c);
      se += __expf(v - m);
      const unsigned kc = ce_sort_key(v);
      above += (kc > ky || (kc == ky && c > (int)y)) ? 1 : 0;
    }
    above = ce_wave_sum_int(above);
    if (lane == 0) redn[w] = above;
  } else {
    for (int c = threadIdx.x; c < K; c += 256) se += __expf(ce_ld(xr, c) - m);
  }
  se = ce_wave_sum(se);
  if (lane == 0) red[0][w] = se;
  __syncthreads();
  if (threadIdx.x == 0) {
    se = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const float l = m + __logf(se);
    const int64_t y = labels[r];
    const bool y_ok = y >= 0 && y < K;
    float xy = y_ok ? ce_ld(xr, (long long)y) : 0.f;
    if (mix) {
      const int64_t y1 = mix[r];
      const float rho = ratio[r];
      const float x1 = (y1 >= 0 && y1 < K) ? ce_ld(xr, (long long)y1) : 0.f;
      xy = rho * xy + (1.f - rho) * x1;
    }
    lse[r] = l;
    row_loss[r] = l - (1.f - alpha) * xy - (alpha / (float)K) * sx;
    if constexpr (RANK) rank[r] = y_ok ? ((redn[0] + redn[1]) + redn[2]) + redn[3] : K;
  }
}

// the mean over rows, summed in row order by one workgroup (deterministic), and (RANK) the fractions
// of rows whose label ranks in the top 1 / top 5: integer counts, so their order does not matter
template <bool RANK>
__global__ __launch_bounds__(256) void ce_mean_kernel(const float* __restrict__ row_loss,
                                                      const int* __restrict__ rank, int R,
                                                      float* __restrict__ loss, float* __restrict__ top) {
  __shared__ float part[256];
  __shared__ int hit[2][256];   // (RANK only)
  // thread t sums the contiguous rows [t * per, (t + 1) * per), then thread 0 adds the 256 parts in order
  const int per = (R + 255) / 256;
  float s = 0.f;
  int h1 = 0, h5 = 0;
  for (int r = threadIdx.x * per; r < min(R, (threadIdx.x + 1) * per); ++r) {
    s += row_loss[r];
    if constexpr (RANK) {
      h1 += rank[r] < 1;
      h5 += rank[r] < 5;
    }
  }
  part[threadIdx.x] = s;
  if constexpr (RANK) {
    hit[0][threadIdx.x] = h1;
    hit[1][threadIdx.x] = h5;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    int t1 = 0, t5 = 0;
    for (int i = 0; i < 256; ++i) {
      t += part[i];
      if constexpr (RANK) {
        t1 += hit[0][i];
        t5 += hit[1][i];
      }
    }
    *loss = t / (float)R;
    if constexpr (RANK) {
      top[0] = (float)t1 / (float)R;
      top[1] = (float)t5 / (float)R;
    }
  }
}

// backward, one workgroup per row.  MIX == (mix != nullptr); MIX == false is rho = 1 and no second
// label, (1 - alpha) (1 + 0), compiled without the second compare and select per element (with mix a
// run-time pointer the one-label backward measured 0.12 us over the former smoothed kernel's 3.34 us
// at 128 x 1000 bf16, twice that kernel's own run-to-run spread: profiles/loss_unify_ab.txt)
template <typename T, bool MIX>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const T* __restrict__ x, long long ld,
                                                     const int64_t* __restrict__ labels,
                                                     const int64_t* __restrict__ mix, const float* __restrict__ ratio,
                                                     int R, int K, float alpha, const float* __restrict__ lse,
                                                     const float* __restrict__ gloss, T* __restrict__ dx,
                                                     long long ldd) {
  const int r = blockIdx.x;
  const float g = *gloss / (float)R, l = lse[r], off = alpha / (float)K;
  const int64_t y = labels[r], y1 = MIX ? mix[r] : -1;
  const float rho = MIX ? ratio[r] : 1.f;
  const T* xr = x + (long long)r * ld;
  T* dr = dx + (long long)r * ldd;
  for (int c = threadIdx.x; c < K; c += 256) {
    const float p = __expf(ce_ld(xr, c) - l);
    const float t = MIX ? (1.f - alpha) * ((c == y ? rho : 0.f) + (c == y1 ? 1.f - rho : 0.f))
                        : (c == y ? 1.f - alpha : 0.f);
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

// adamw.h -- the optimizer update of the data-parallel training step, one launch for every
// parameter of the model (the §8f "DP train-step harness" row).
//
// Reference: train.py:25-27,229-233 builds optax.adamw (b1 0.9, b2 0.999, eps 1e-8, decoupled
// weight decay 1e-4) and applies it once per batch (train.py:94-100; survey D9: descent, not the
// reference chain's ascent).  The update follows torch.optim.AdamW's order of operations, which
// the host-side harness used before this kernel (train.py) and the parity test compares against:
//   p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v = b2 v + (1 - b2) g^2;
//   p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound elementwise work (28 bytes per parameter: read p, g, m, v, write p, m, v): the
// parameters are cut into 2048-element chunks (one 256-thread workgroup, 8 consecutive elements
// per thread as two 16-byte accesses); a device-resident chunk table built once by the host
// names each chunk's four pointers, so ~150 tensors cost one launch instead of torch's five
// multi-tensor launches.  The step counter lives in device memory (incremented by a one-thread
// kernel in the same stream) so a captured HIP graph replays the correct bias corrections.
//
// The reference's full chain (train.py:22-27,214-220: clip_by_global_norm, scale_by_adam,
// additive_weight_decay, scale_by_schedule(warmup_cosine_decay_schedule)) needs two values that
// change every step, the learning rate and the clip factor.  They live in a device buffer
// hyper = {lr_t, clip_scale, grad_norm, -}: adamw_sumsq_kernel reduces the flat gradient buffer
// to one fp64 partial per workgroup (no atomics: the order of summation is fixed by n and the
// base alignment alone), adamw_prepare_kernel (one workgroup, in place of the tick) adds the
// partials, writes hyper, evaluates the schedule at the device step count and increments it, and
// the *_dev update kernels read lr_t and clip_scale from hyper -- so a captured graph replays
// with this step's rate and this step's clip.
#pragma once
#include "common.h"

namespace sae {

constexpr int kAdamwChunk = 2048;   // elements per chunk (256 threads x 8)
constexpr int kAdamwNormSpan = 16384;       // gradient elements per workgroup of the norm pass (256 x 16 float4)
constexpr int kAdamwPreparePass = 256;      // partials the prepare kernel adds per pass (one per thread)

struct AdamwSchedule {   // mirrors sae_lr_schedule
  int32_t kind;
  float init, peak, end;
  int32_t warmup_steps, decay_steps;
};

// hyper[0] = lr_t, [1] = clip_scale, [2] = grad_norm, [3] unused
constexpr int kHyperLr = 0, kHyperClip = 1, kHyperNorm = 2;

struct AdamwChunk {
  float* p;
  const float* g;
  float* m;
  float* v;
  int32_t n;       // elements in this chunk (<= kAdamwChunk)
  int32_t vec;     // all four pointers 16-byte aligned and n == kAdamwChunk
};

__global__ void adamw_tick_kernel(int32_t* step) {
  if (threadIdx.x == 0) *step += 1;
}

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float decay, float b1c, float b2,
                                          float b2c, float step_size, float inv_bc2s, float eps) {
  p *= decay;
  m = __builtin_fmaf(b1c, g - m, m);                 // torch lerp (weight < 0.5): m + w (g - m)
  v = __builtin_fmaf(b2, v, b2c * g * g);            // v * b2 + (1 - b2) g^2 (addcmul)
  const float denom = __builtin_sqrtf(v) * inv_bc2s + eps;
  p = __builtin_fmaf(-step_size, m / denom, p);
}

struct AdamwConst {
  float decay, b1c, b2, b2c, step_size, inv_bc2s, eps;
  float gscale = 1.f;   // the clip factor every gradient is multiplied by (the *_dev kernels only)
  // lr_t and clip_scale from the device buffer the prepare kernel wrote
  __device__ __forceinline__ AdamwConst(const int32_t* step, const float* hyper, float b1, float b2_, float eps_,
                                        float wd)
      : AdamwConst(step, hyper[kHyperLr], b1, b2_, eps_, wd) {
    gscale = hyper[kHyperClip];
  }
  __device__ __forceinline__ AdamwConst(const int32_t* step, float lr, float b1, float b2_, float eps_, float wd) {
    const float t = (float)(*step);
    const float bc1 = 1.f - __builtin_powf(b1, t), bc2 = 1.f - __builtin_powf(b2_, t);
    step_size = lr / bc1;
    inv_bc2s = 1.f / __builtin_sqrtf(bc2);
    decay = 1.f - lr * wd;
    b1c = 1.f - b1;
    b2 = b2_;
    b2c = 1.f - b2_;
    eps = eps_;
  }
};

// g * clip_scale, rounded to fp32 before adamw_one sees it (never contracted into its FMAs, so the
// chunk and the tile path keep giving the same bits); kClip false: the by-value kernels, g as is
template <bool kClip>
__device__ __forceinline__ float adamw_clip(float g, float s) {
#pragma clang fp contract(off)
  return kClip ? g * s : g;
}
template <bool kClip>
__device__ __forceinline__ float4 adamw_clip(float4 g, float s) {
  return float4{adamw_clip<kClip>(g.x, s), adamw_clip<kClip>(g.y, s), adamw_clip<kClip>(g.z, s),
                adamw_clip<kClip>(g.w, s)};
}

// one 2048-element chunk of the flat table
template <bool kClip = false>
__device__ __forceinline__ void adamw_chunk(const AdamwChunk& c, const AdamwConst& k) {
  const float decay = k.decay, b1c = k.b1c, b2 = k.b2, b2c = k.b2c, step_size = k.step_size,
              inv_bc2s = k.inv_bc2s, eps = k.eps;
  const int i0 = threadIdx.x * 8;
  if (c.vec) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = i0 + 4 * h;
      float4 p = *reinterpret_cast<const float4*>(c.p + i);
      const float4 g = adamw_clip<kClip>(*reinterpret_cast<const float4*>(c.g + i), k.gscale);
      float4 m = *reinterpret_cast<const float4*>(c.m + i);
      float4 v = *reinterpret_cast<const float4*>(c.v + i);
      adamw_one(p.x, g.x, m.x, v.x, decay, b1c, b2, b2c, step_size, inv_bc2s, eps);
      adamw_one(p.y, g.y, m.y, v.y, decay, b1c, b2, b2c, step_size, inv_bc2s, eps);
      adamw_one(p.z, g.z, m.z, v.z, decay, b1c, b2, b2c, step_size, inv_bc2s, eps);
      adamw_one(p.w, g.w, m.w, v.w, decay, b1c, b2, b2c, step_size, inv_bc2s, eps);
      *reinterpret_cast<float4*>(c.p + i) = p;
      *reinterpret_cast<float4*>(c.m + i) = m;
      *reinterpret_cast<float4*>(c.v + i) = v;
    }
  } else {
    for (int i = i0; i < i0 + 8 && i < c.n; ++i) {
      float p = c.p[i], m = c.m[i], v = c.v[i];
      adamw_one(p, adamw_clip<kClip>(c.g[i], k.gscale), m, v, decay, b1c, b2, b2c, step_size, inv_bc2s, eps);
      c.p[i] = p;
      c.m[i] = m;
      c.v[i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(const AdamwChunk* __restrict__ chunks,
                                                    const int32_t* __restrict__ step, float lr, float b1,
                                                    float b2, float eps, float wd) {
  adamw_chunk(chunks[blockIdx.x], AdamwConst(step, lr, b1, b2, eps, wd));
}

__global__ __launch_bounds__(256) void adamw_dev_kernel(const AdamwChunk* __restrict__ chunks,
                                                        const int32_t* __restrict__ step,
                                                        const float* __restrict__ hyper, float b1, float b2,
                                                        float eps, float wd) {
  adamw_chunk<true>(chunks[blockIdx.x], AdamwConst(step, hyper, b1, b2, eps, wd));
}

// A 64 x 64 tile of a Dense kernel [K][N]: the AdamW update (identical arithmetic to the chunk
// path) plus the bf16 compute copies the next forward reads, w16 [K][ld16] at column col0 and its
// transpose wt16 [.][ldT] at row col0 (the tile goes through LDS for the transposed 8-byte
// stores) -- what sae_weight_cast_multi does at the start of every forward, moved into the update
// that produces the values.
struct AdamwCastTile {
  float* p;
  const float* g;
  float* m;
  float* v;
  __bf16* w16;
  __bf16* wt16;
  int32_t K, N, ld16, ldT, col0, k0, n0, pad;
};

template <bool kClip = false>
__device__ __forceinline__ void adamw_cast_tile(const AdamwCastTile& c, const AdamwConst& k, float (*tile)[65]) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = t + 256 * q, row = i >> 4, c4 = i & 15;
    const int kk = c.k0 + row, n = c.n0 + 4 * c4;
    float4 pv = {0.f, 0.f, 0.f, 0.f};
    if (kk < c.K && n < c.N) {
      const long long off = (long long)kk * c.N + n;
      pv = *reinterpret_cast<const float4*>(c.p + off);
      const float4 g = adamw_clip<kClip>(*reinterpret_cast<const float4*>(c.g + off), k.gscale);
      float4 m = *reinterpret_cast<const float4*>(c.m + off);
      float4 v = *reinterpret_cast<const float4*>(c.v + off);
      adamw_one(pv.x, g.x, m.x, v.x, k.decay, k.b1c, k.b2, k.b2c, k.step_size, k.inv_bc2s, k.eps);
      adamw_one(pv.y, g.y, m.y, v.y, k.decay, k.b1c, k.b2, k.b2c, k.step_size, k.inv_bc2s, k.eps);
      adamw_one(pv.z, g.z, m.z, v.z, k.decay, k.b1c, k.b2, k.b2c, k.step_size, k.inv_bc2s, k.eps);
      adamw_one(pv.w, g.w, m.w, v.w, k.decay, k.b1c, k.b2, k.b2c, k.step_size, k.inv_bc2s, k.eps);
      *reinterpret_cast<float4*>(c.p + off) = pv;
      *reinterpret_cast<float4*>(c.m + off) = m;
      *reinterpret_cast<float4*>(c.v + off) = v;
      if (c.w16)
        *reinterpret_cast<bf16x4*>(c.w16 + (long long)kk * c.ld16 + c.col0 + n) =
            bf16x4{(__bf16)pv.x, (__bf16)pv.y, (__bf16)pv.z, (__bf16)pv.w};
    }
    tile[row][4 * c4] = pv.x;
    tile[row][4 * c4 + 1] = pv.y;
    tile[row][4 * c4 + 2] = pv.z;
    tile[row][4 * c4 + 3] = pv.w;
  }
  if (!c.wt16) return;   // (uniform per tile)
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = t + 256 * q, nn = i >> 4, kq = i & 15;
    const int n = c.n0 + nn, kk = c.k0 + 4 * kq;
    if (n < c.N && kk < c.K)
      *reinterpret_cast<bf16x4*>(c.wt16 + (long long)(c.col0 + n) * c.ldT + kk) =
          bf16x4{(__bf16)tile[4 * kq][nn], (__bf16)tile[4 * kq + 1][nn], (__bf16)tile[4 * kq + 2][nn],
                 (__bf16)tile[4 * kq + 3][nn]};
  }
}

// workgroups [0, n_chunks): the flat chunks; [n_chunks, n_chunks + n_tiles): the Dense-kernel tiles
__global__ __launch_bounds__(256) void adamw_cast_kernel(const AdamwChunk* __restrict__ chunks, int n_chunks,
                                                         const AdamwCastTile* __restrict__ tiles,
                                                         const int32_t* __restrict__ step, float lr, float b1,
                                                         float b2, float eps, float wd) {
  __shared__ float tile[64][65];
  const AdamwConst k(step, lr, b1, b2, eps, wd);
  const int b = blockIdx.x;
  if (b < n_chunks) adamw_chunk(chunks[b], k);
  else adamw_cast_tile(tiles[b - n_chunks], k, tile);
}

__global__ __launch_bounds__(256) void adamw_cast_dev_kernel(const AdamwChunk* __restrict__ chunks, int n_chunks,
                                                             const AdamwCastTile* __restrict__ tiles,
                                                             const int32_t* __restrict__ step,
                                                             const float* __restrict__ hyper, float b1, float b2,
                                                             float eps, float wd) {
  __shared__ float tile[64][65];
  const AdamwConst k(step, hyper, b1, b2, eps, wd);
  const int b = blockIdx.x;
  if (b < n_chunks) adamw_chunk<true>(chunks[b], k);
  else adamw_cast_tile<true>(tiles[b - n_chunks], k, tile);
}

// ---- global gradient norm (optax.clip_by_global_norm, reference train.py:22-24) and the schedule
// Sum of a workgroup's 256 fp64 values in a fixed order (xor butterfly inside each wave, then the
// four wave sums in wave order); the result is valid in thread 0.
__device__ __forceinline__ double adamw_block_sum(double a, double* wave_sums) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = a;
  __syncthreads();
  return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
}

// partial[b] = sum of g[i]^2 over i in [b span, min(n, (b + 1) span)): every square is exact in
// fp64 (a 24-bit significand squared has 48 bits) and all sums are fp64, so the only roundings
// are fp64 adds.  HBM-bound (4 bytes and two fp64 operations per element).  A 16-byte aligned base
// takes 16-byte loads (float4 j * 256 + t of the span: coalesced) with at most three scalar tail
// elements in the last workgroup; any other base takes coalesced scalar loads.
__global__ __launch_bounds__(256) void adamw_sumsq_kernel(const float* __restrict__ g, long long n,
                                                          double* __restrict__ partial) {
  __shared__ double wave_sums[4];
  const int t = threadIdx.x;
  const long long lo = (long long)blockIdx.x * kAdamwNormSpan;
  const int cnt = (int)((n - lo) < (long long)kAdamwNormSpan ? (n - lo) : (long long)kAdamwNormSpan);
  const float* gb = g + lo;
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  if (((uintptr_t)g & 15) == 0) {
    const float4* g4 = reinterpret_cast<const float4*>(gb);
    const int nv = cnt >> 2;
    if (nv == kAdamwNormSpan / 4) {   // a full span: four loads in flight per thread
#pragma unroll
      for (int j = 0; j < 16; j += 4) {
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = g4[(j + u) * 256 + t];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a0 = __builtin_fma((double)r[u].x, (double)r[u].x, a0);
          a1 = __builtin_fma((double)r[u].y, (double)r[u].y, a1);
          a2 = __builtin_fma((double)r[u].z, (double)r[u].z, a2);
          a3 = __builtin_fma((double)r[u].w, (double)r[u].w, a3);
        }
      }
    } else {
      for (int i = t; i < nv; i += 256) {
        const float4 r = g4[i];
        a0 = __builtin_fma((double)r.x, (double)r.x, a0);
        a1 = __builtin_fma((double)r.y, (double)r.y, a1);
        a2 = __builtin_fma((double)r.z, (double)r.z, a2);
        a3 = __builtin_fma((double)r.w, (double)r.w, a3);
      }
      const int i = 4 * nv + t;   // the tail: at most three elements
      if (i < cnt) a0 = __builtin_fma((double)gb[i], (double)gb[i], a0);
    }
  } else {
    for (int i = t; i < cnt; i += 256) a0 = __builtin_fma((double)gb[i], (double)gb[i], a0);
  }
  const double s = adamw_block_sum((a0 + a1) + (a2 + a3), wave_sums);
  if (t == 0) partial[blockIdx.x] = s;
}

// warmup_cosine_decay_schedule as optax composes it (linear_schedule joined with
// cosine_decay_schedule at warmup_steps; reference train.py:214-220), at count = updates applied
__device__ __forceinline__ float adamw_schedule(const AdamwSchedule& s, int count) {
  if (s.kind == 0) return s.peak;
  if (count < s.warmup_steps) return s.init + (s.peak - s.init) * (float)count / (float)s.warmup_steps;
  const int D = s.decay_steps - s.warmup_steps;
  const int c = count - s.warmup_steps < D ? count - s.warmup_steps : D;
  const float alpha = s.end / s.peak;
  const float cosine = 0.5f * (1.f + cosf(3.14159265358979323846f * (float)c / (float)D));
  return s.peak * ((1.f - alpha) * cosine + alpha);
}

// One workgroup, in place of adamw_tick_kernel: adds the norm pass's partials (thread t adds
// partials t, t + 256, ... in increasing index, then the fixed-order block sum), writes grad_norm
// and optax's clip factor, evaluates the schedule at *step and increments *step.  n_partials == 0
// (no norm pass): grad_norm 0, clip_scale 1.  A NaN norm gives a NaN clip factor (tested on the
// bits: the library is compiled without NaN-honouring comparisons), an infinite one gives 0.
__global__ __launch_bounds__(256) void adamw_prepare_kernel(const double* __restrict__ partial, int n_partials,
                                                            float max_norm, AdamwSchedule sched,
                                                            int32_t* __restrict__ step, float* __restrict__ hyper) {
  __shared__ double wave_sums[4];
  double a = 0.;
  for (int i = threadIdx.x; i < n_partials; i += kAdamwPreparePass) a += partial[i];
  const double total = adamw_block_sum(a, wave_sums);
  if (threadIdx.x != 0) return;
  const float norm = (float)__builtin_sqrt(total);
  const bool nan = (__float_as_uint(norm) & 0x7fffffffu) > 0x7f800000u;
  hyper[kHyperNorm] = norm;
  hyper[kHyperClip] = nan ? norm : (norm < max_norm ? 1.f : max_norm / norm);
  const int32_t count = *step;
  hyper[kHyperLr] = adamw_schedule(sched, count);
  hyper[3] = 0.f;
  *step = count + 1;
}

}  // namespace sae

// tokens.h -- the encoder input of ViT / DeiT: class token + patch tokens + absolute position
// embedding, forward and backward (the glue between the §8f patch-embedding row and the first
// encoder block).
//
// Reference: models/vit.py:82-85 (cls = tile(param, [b, 1, 1]); x = concatenate([cls, x], 1)) and
// vit.py:46 + layers/position_embed.py:48 (AddAbsPosEmbed: x + pos_embed), with the patch tokens
// promoted from the compute dtype to the fp32 residual stream:
//     x[b, 0, c] = cls[c] + pos[0, c];   x[b, 1 + p, c] = float(tok[b, p, c]) + pos[1 + p, c]
// Backward: dtok[b, p] = bf16(dx[b, 1 + p]), dpos[n] = sum_b dx[b, n], dcls = dpos[0].  One pass
// each way instead of the upcast, concatenate and add kernels (and their backward: slice, cast and
// two batch reductions).  HBM-bound: 2 B read + 4 B written per element forward, 4 B read + 2 B
// written backward.
// Dropout forms (vit.py:47, nn.Dropout on the encoder input; drop_rows.h over rows b (L + 1) + n,
// columns E): x = (concat(cls, tok) + pos) * keep / pk, and g = dx * keep / pk in place of dx in the
// backward.  A thread's 4 channels are one Philox word; each thread runs its own call (the quads of
// a flat index do not line up with the 16-column blocks when E / 4 is not a multiple of 4, and
// both kernels run once per step).
#pragma once
#include "common.h"
#include "drop_rows.h"

namespace sae {

__device__ __forceinline__ f32x4 tokens_drop_scale(const DropKey& dk, const DropRows& d, long long row, int c4) {
  const unsigned long long r = (unsigned long long)(d.row0 + row * d.row_step);
  return drop_scale4(drop_word(drop_rows_call(dk, r, (unsigned)c4 >> 2), (unsigned)c4 & 3u), d.thr, d.inv);
}

// one thread per 4 consecutive channels of one token
template <bool DROP>
__device__ __forceinline__ void tokens_fwd_body(const __bf16* __restrict__ tok, const float* __restrict__ cls,
                                                const float* __restrict__ pos, float* __restrict__ x, int B, int L,
                                                int E, const DropRows& d) {
  const int E4 = E / 4, N = L + 1;
  DropKey dk = {};
  if constexpr (DROP) dk = drop_key(d.rng, d.stream_id);
  const long long total = (long long)B * N * E4;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c4 = (int)(i % E4);
    const long long bn = i / E4;
    const int n = (int)(bn % N);
    const long long b = bn / N;
    const f32x4 p = reinterpret_cast<const f32x4*>(pos)[(long long)n * E4 + c4];
    f32x4 v;
    if (n == 0) {
      v = reinterpret_cast<const f32x4*>(cls)[c4];
    } else {
      const uint2 t = reinterpret_cast<const uint2*>(tok)[(b * L + n - 1) * E4 + c4];
      v = f32x4{__uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u), __uint_as_float(t.y << 16),
                __uint_as_float(t.y & 0xffff0000u)};
    }
    if constexpr (DROP) reinterpret_cast<f32x4*>(x)[i] = (v + p) * tokens_drop_scale(dk, d, bn, c4);
    else reinterpret_cast<f32x4*>(x)[i] = v + p;
  }
}
__global__ __launch_bounds__(256) void tokens_fwd_kernel(const __bf16* __restrict__ tok, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, float* __restrict__ x, int B,
                                                         int L, int E) {
  tokens_fwd_body<false>(tok, cls, pos, x, B, L, E, DropRows{});
}
__global__ __launch_bounds__(256) void tokens_fwd_drop_kernel(const __bf16* __restrict__ tok,
                                                              const float* __restrict__ cls,
                                                              const float* __restrict__ pos, float* __restrict__ x,
                                                              int B, int L, int E, DropRows d) {
  tokens_fwd_body<true>(tok, cls, pos, x, B, L, E, d);
}

// one workgroup per token position n: E / 4 channel groups x G batch groups (G = blockDim / (E/4));
// batch group g sums b = g, g + G, ... and the G partial sums are added in group order
// (deterministic).  LDS: G * E * 4 bytes.
template <bool DROP>
__device__ __forceinline__ void tokens_bwd_body(const float* __restrict__ dx, __bf16* __restrict__ dtok,
                                                float* __restrict__ dcls, float* __restrict__ dpos, int B, int L,
                                                int E, const DropRows& d) {
  extern __shared__ f32x4 part[];   // [G][E4]
  DropKey dk = {};
  if constexpr (DROP) dk = drop_key(d.rng, d.stream_id);
  const int E4 = E / 4, N = L + 1, n = blockIdx.x;
  const int G = blockDim.x / E4;
  const int c4 = threadIdx.x % E4, g = threadIdx.x / E4;
  if (g < G) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = g; b < B; b += G) {
      f32x4 v = reinterpret_cast<const f32x4*>(dx)[((long long)b * N + n) * E4 + c4];
      if constexpr (DROP) v *= tokens_drop_scale(dk, d, (long long)b * N + n, c4);
      acc += v;
      if (n > 0) {
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        const bf16x4 t = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
        reinterpret_cast<bf16x4*>(dtok)[((long long)b * L + n - 1) * E4 + c4] = t;
      }
    }
    part[g * E4 + c4] = acc;
  }
  __syncthreads();
  if (g == 0) {
    f32x4 s = part[c4];
    for (int q = 1; q < G; ++q) s += part[q * E4 + c4];
    reinterpret_cast<f32x4*>(dpos)[(long long)n * E4 + c4] = s;
    if (n == 0 && dcls) reinterpret_cast<f32x4*>(dcls)[c4] = s;
  }
}
__global__ __launch_bounds__(1024) void tokens_bwd_kernel(const float* __restrict__ dx, __bf16* __restrict__ dtok,
                                                          float* __restrict__ dcls, float* __restrict__ dpos, int B,
                                                          int L, int E) {
  tokens_bwd_body<false>(dx, dtok, dcls, dpos, B, L, E, DropRows{});
}
__global__ __launch_bounds__(1024) void tokens_bwd_drop_kernel(const float* __restrict__ dx, __bf16* __restrict__ dtok,
                                                               float* __restrict__ dcls, float* __restrict__ dpos,
                                                               int B, int L, int E, DropRows d) {
  tokens_bwd_body<true>(dx, dtok, dcls, dpos, B, L, E, d);
}

}  // namespace sae

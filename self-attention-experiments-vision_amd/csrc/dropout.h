// dropout.h -- attention-probability dropout (attention.py:54-58: nn.Dropout on the softmax output
// before the AV product) as a pure function of counters.  Forward and backward regenerate the same
// keep mask; nothing is stored, and the mask does not depend on the kernel or tile shape serving
// the call:
//   T        = clamp(lrintf(rate * 256), 0, 255),  keep probability pk = (256 - T) / 256
//   (k0, k1) = words 0, 1 of Philox4x32-10(counter (lo32(offset), hi32(offset), stream_id, 0),
//                                          key (lo32(seed), hi32(seed)))
//   W        = Philox4x32-10(counter (k >> 2, q >> 2, b * H + h, 0), key (k0, k1))
//   keep(b, h, q, k) = ((W[q & 3] >> (8 * (k & 3))) & 0xff) >= T
// seed = rng[0] and offset = rng[1] are read from device memory by every kernel, so a captured
// graph replays with a fresh mask once sae_dropout_advance has bumped the offset on the stream.
//
// One Philox call covers a 4 x 4 block of (q, k).  The score accumulator of a 32 x 32 MFMA holds,
// per lane, one index of the lane axis and four groups of 4 consecutive indices of the register
// axis (row_of), and the four lanes of a quad share (lane index >> 2): each lane of a quad runs
// the call of one of the four groups and the quad exchanges the words with DPP quad_perm -- one
// call per 16 elements, none wasted, with the query on the lane (forward, dQ) or the key (dK / dV).
#pragma once
#include <type_traits>

#include "common.h"

namespace sae {

struct DropKey {
  unsigned k0, k1;
};

__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                               unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return uint4{c0, c1, c2, c3};
}

// the call's key: wave-uniform (scalar loads of the device state, the same ten rounds in every lane)
__device__ __forceinline__ DropKey drop_key(const unsigned long long* rng, unsigned stream_id) {
  const unsigned long long seed = rng[0], off = rng[1];
  const uint4 w = philox4x32_10((unsigned)off, (unsigned)(off >> 32), stream_id, 0u, (unsigned)seed,
                                (unsigned)(seed >> 32));
  return DropKey{w.x, w.y};
}

__device__ __forceinline__ bool drop_keep(const DropKey& dk, unsigned thr, unsigned bh, unsigned q, unsigned k) {
  const uint4 w = philox4x32_10(k >> 2, q >> 2, bh, 0u, dk.k0, dk.k1);
  const unsigned ww[4] = {w.x, w.y, w.z, w.w};
  return ((ww[q & 3] >> (8 * (k & 3))) & 0xffu) >= thr;
}

template <int G> __device__ __forceinline__ unsigned quad_bcast(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, G * 0x55, 0xf, 0xf, false);
}

// Keep bits of one 32 x 32 accumulator tile: bit r <-> accumulator register r, whose register-axis
// index is 4 * reg4 + (r & 3) + 8 * (r >> 2) (reg4 carries the lane half: row_of(r, h) = .. + 4h).
// QLANE: the lane axis is the query (lidx = q, register axis = keys), otherwise the key.
// lidx must be congruent to the lane id mod 4, and the whole quad must be executing.
template <bool QLANE>
__device__ __forceinline__ unsigned drop_keep16(const DropKey& dk, unsigned thr, unsigned bh, int lidx, int reg4) {
  const unsigned i = (unsigned)lidx & 3u;
  const unsigned mine = (unsigned)reg4 + 2u * i, lb = (unsigned)lidx >> 2;   // this lane's group g = i
  const uint4 w = QLANE ? philox4x32_10(mine, lb, bh, 0u, dk.k0, dk.k1) : philox4x32_10(lb, mine, bh, 0u, dk.k0, dk.k1);
  unsigned keep = 0;
  auto group = [&](auto gc) {
    constexpr int g = decltype(gc)::value;
    const unsigned w0 = quad_bcast<g>(w.x), w1 = quad_bcast<g>(w.y), w2 = quad_bcast<g>(w.z), w3 = quad_bcast<g>(w.w);
    if constexpr (QLANE) {   // word q & 3, one byte per key
      const unsigned ww = i == 0 ? w0 : (i == 1 ? w1 : (i == 2 ? w2 : w3));
#pragma unroll
      for (int j = 0; j < 4; ++j) keep |= (((ww >> (8 * j)) & 0xffu) >= thr ? 1u : 0u) << (4 * g + j);
    } else {                 // byte k & 3 of the word of each query
      const unsigned sh = 8u * i;
      keep |= (((w0 >> sh) & 0xffu) >= thr ? 1u : 0u) << (4 * g);
      keep |= (((w1 >> sh) & 0xffu) >= thr ? 1u : 0u) << (4 * g + 1);
      keep |= (((w2 >> sh) & 0xffu) >= thr ? 1u : 0u) << (4 * g + 2);
      keep |= (((w3 >> sh) & 0xffu) >= thr ? 1u : 0u) << (4 * g + 3);
    }
  };
  group(std::integral_constant<int, 0>{});
  group(std::integral_constant<int, 1>{});
  group(std::integral_constant<int, 2>{});
  group(std::integral_constant<int, 3>{});
  return keep;
}

}  // namespace sae

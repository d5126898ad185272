// drop_rows.h -- hidden-state dropout (models/vit.py:47, attention.py out_dropout_rate, ff.py:30,32:
// nn.Dropout(rate = dropout_rate)) on a row-major activation [rows][cols], as a pure function of
// counters like the attention mask of dropout.h (same T, pk, device state and drop_key):
//   W              = Philox4x32-10(counter (col >> 4, lo32(row), hi32(row), 1), key (k0, k1))
//   keep(row, col) = ((W[(col >> 2) & 3] >> (8 * (col & 3))) & 0xff) >= T
//   row            = row0 + i * row_step   (64-bit; i = the row the kernel is working on)
//   y              = x * keep / pk
// One call covers 16 consecutive columns of one row; counter word 3 = 1 keeps it apart from the
// attention mask (word 3 = 0) of the same key.  row0 / row_step let a kernel that works on a strided
// subset of the rows (the class-token rows b * N of cls_add_layer_norm) draw the mask of the full
// tensor.  The mask does not depend on the kernel applying it: the LayerNorm (ln.h), tokens
// (tokens.h) and GELU GEMM (gemm_nt.h, gemm8.h) forms and the standalone kernels (misc.hip) agree.
#pragma once
#include <type_traits>

#include "dropout.h"

namespace sae {

// what every dropout form of a kernel carries
struct DropRows {
  const unsigned long long* rng;   // device {seed, offset}
  unsigned stream_id, thr;         // thr = T
  float inv;                       // 1 / pk = 256 / (256 - T)
  long long row0, row_step;
};

// host: thr = T from rows_drop_check (host.h)
inline DropRows make_drop_rows(const uint64_t* rng, uint32_t stream_id, unsigned thr, long long row0,
                               long long row_step) {
  DropRows d;
  d.rng = reinterpret_cast<const unsigned long long*>(rng);
  d.stream_id = stream_id;
  d.thr = thr;
  d.inv = 256.f / (float)(256 - (int)thr);
  d.row0 = row0;
  d.row_step = row_step;
  return d;
}

__device__ __forceinline__ uint4 drop_rows_call(const DropKey& dk, unsigned long long row, unsigned blk) {
  return philox4x32_10(blk, (unsigned)row, (unsigned)(row >> 32), 1u, dk.k0, dk.k1);
}

__device__ __forceinline__ unsigned drop_word(const uint4& w, unsigned i) {
  return i == 0 ? w.x : (i == 1 ? w.y : (i == 2 ? w.z : w.w));
}

// keep / pk of the 4 columns whose bytes are `word` (columns 4 j .. 4 j + 3 of a 16-column block)
__device__ __forceinline__ f32x4 drop_scale4(unsigned word, unsigned thr, float inv) {
  return f32x4{(word & 0xffu) >= thr ? inv : 0.f, ((word >> 8) & 0xffu) >= thr ? inv : 0.f,
               ((word >> 16) & 0xffu) >= thr ? inv : 0.f, (word >> 24) >= thr ? inv : 0.f};
}

// one element (the mask kernel)
__device__ __forceinline__ bool drop_rows_keep(const DropKey& dk, unsigned thr, unsigned long long row, unsigned col) {
  const unsigned w = drop_word(drop_rows_call(dk, row, col >> 4), (col >> 2) & 3u);
  return ((w >> (8 * (col & 3u))) & 0xffu) >= thr;
}

// The words of a wave that holds one row as float4 chunks c = lane + 64 k (columns 4 c .. 4 c + 3,
// k < NV): chunk c is word c & 3 = lane & 3 of block c >> 2 = (lane >> 2) + 16 k, so the four lanes
// of a quad need the four words of ONE call per k.  Lane i of the quad runs the call of chunk row
// k = i and the quad exchanges the words with DPP quad_perm: one call per lane for up to 4 chunks
// (16 columns per call, none wasted at NV = 4).  The whole wave must be executing.
template <int NV>
__device__ __forceinline__ void drop_wave_words(const DropKey& dk, unsigned long long row, int lane, unsigned (&w)[NV]) {
  static_assert(NV >= 1 && NV <= 4, "one call per lane covers up to four chunk rows");
  const unsigned i = (unsigned)lane & 3u;
  const uint4 p = drop_rows_call(dk, row, ((unsigned)lane >> 2) + 16u * i);
  auto pick = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const uint4 q = {quad_bcast<k>(p.x), quad_bcast<k>(p.y), quad_bcast<k>(p.z), quad_bcast<k>(p.w)};
    return drop_word(q, i);
  };
  w[0] = pick(std::integral_constant<int, 0>{});
  if constexpr (NV > 1) w[1] = pick(std::integral_constant<int, 1>{});
  if constexpr (NV > 2) w[2] = pick(std::integral_constant<int, 2>{});
  if constexpr (NV > 3) w[3] = pick(std::integral_constant<int, 3>{});
}

}  // namespace sae

// gelu.h -- the tanh-GELU and its derivative on one fp32 element: the FF GEMM epilogues of gemm_nt.h
// and the BatchNorm + GELU rows of bn_rows.h compute the activation through these, and only these.
#pragma once
#include "common.h"

namespace sae {

// tanh-GELU (Flax nn.gelu default; torch approximate="tanh"): 0.5 x (1 + tanh(y)),
// y = sqrt(2/pi) (x + 0.044715 x^3) = x * sigmoid(2y)
constexpr float kGeluB = 0.7978845608028654f;
constexpr float kGeluK = 0.044715f;

__device__ __forceinline__ float gelu_sig(float x) {   // sigmoid(2y)
  const float y2 = x * (kGeluB + (kGeluB * kGeluK) * x * x);
  return __builtin_amdgcn_rcpf(1.f + ex2(-2.f * kLog2e * y2));
}
__device__ __forceinline__ float gelu_f(float x) { return x * gelu_sig(x); }
__device__ __forceinline__ float dgelu_f(float x) {
  const float s = gelu_sig(x);
  return s + 2.f * x * s * (1.f - s) * (kGeluB + (3.f * kGeluB * kGeluK) * x * x);
}

}  // namespace sae

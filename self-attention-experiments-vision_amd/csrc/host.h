// host.h -- the host side every translation unit shares: the error string behind sae_last_error,
// argument predicates and the one launch helper.  No allocation, no host synchronisation, no
// global mutable state besides the thread-local error string.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/sae_attn.h"

namespace sae {

extern thread_local std::string g_err;   // one object for the library, defined in misc.hip

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

inline int ok() {
  g_err.clear();
  return SAE_OK;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(SAE_EHIP, "%s: launch failed: %s", what, hipGetErrorString(e));
  return ok();
}

// Kernels asking for more than 64 KiB of dynamic LDS raise their limit once (up to the 160 KiB
// of a gfx950 CU); failure is reported, never silently ignored.
inline int lds_attr(const void* fn, size_t bytes) {
  if (bytes > 160 * 1024) return fail(SAE_EUNSUPPORTED, "kernel needs %zu bytes of LDS (> 160 KiB)", bytes);
  if (bytes <= 64 * 1024) return SAE_OK;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return fail(SAE_EHIP, "hipFuncSetAttribute(%zu B LDS): %s", bytes, hipGetErrorString(e));
  return SAE_OK;
}

// Every kernel launch of the library: grid bound, LDS limit, launch, launch status -- in that order.
// A linear grid comes as a long long and is refused beyond 2^31 - 1 workgroups; the few 2-D / 3-D
// grids (tile rows x tile columns x splits) come as a dim3; an extent the device refuses shows up
// as the launch status.
template <typename... P, typename... A>
int launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
  if (int rc = lds_attr((const void*)kernel, lds)) return rc;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return check_launch(name);
}
template <typename... P, typename... A>
int launch(const char* name, void (*kernel)(P...), long long grid, dim3 block, size_t lds, hipStream_t st,
           A&&... args) {
  if (grid > 0x7fffffffLL) return fail(SAE_EUNSUPPORTED, "grid too large");
  return launch(name, kernel, dim3((unsigned)grid), block, lds, st, args...);
}

// A kernel template over the element type: fn(T*) (a null pointer that only carries the type) with
// T = __bf16 or float by dtype, which the caller has checked to be one of the two.
template <typename F>
int by_dtype(int dtype, F&& fn) {
  return dtype == SAE_DTYPE_BF16 ? fn(static_cast<__bf16*>(nullptr)) : fn(static_cast<float*>(nullptr));
}

// Development A/B knobs, read from the environment only in the dev build (build.py --dev defines
// SAE_DEV_KNOBS); the release library takes the fixed dispatch and never reads the environment on
// a launch path.  Rule: both libraries hold the same set of kernels.  A knob chooses among kernels
// the release launches somewhere, or sets a run-time argument; it never instantiates a kernel of
// its own.  A schedule that lost its A/B is deleted (DESIGN_HISTORY.md, profiles/ and the git
// history keep the measurement), not parked behind a knob.
#ifdef SAE_DEV_KNOBS
inline int dev_knob(const char* name) {
  const char* e = getenv(name);
  if (!e || !*e) return 0;
  return atoi(e[0] == 'v' ? e + 1 : e);
}
#else
constexpr int dev_knob(const char*) { return 0; }
#endif

inline int elem_size(int dtype) { return dtype == SAE_DTYPE_BF16 ? 2 : 4; }

inline bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

// Arguments of the hidden-state dropout entry points (drop_rows.h), checked before any HIP call:
// *thr = T = clamp(lrintf(rate * 256), 0, 255); T == 0 (a rate below 1 / 512) means no dropout and
// the caller forwards to the plain entry point.
inline int rows_drop_check(const char* what, float rate, const uint64_t* rng, int64_t row_step, unsigned* thr) {
  if (!(rate >= 0.f && rate < 1.f)) return fail(SAE_EINVAL, "%s: dropout rate %g is outside [0, 1)", what, (double)rate);
  if (!rng) return fail(SAE_EINVAL, "%s: rng must be non-NULL", what);
  if (row_step < 1) return fail(SAE_EINVAL, "%s: row_step (%lld) must be >= 1", what, (long long)row_step);
  *thr = (unsigned)std::min(255L, std::max(0L, lrintf(rate * 256.f)));
  return SAE_OK;
}

inline int pick_dp(int D) { return D <= 32 ? 32 : (D <= 64 ? 64 : (D <= 128 ? 128 : 0)); }

inline bool strides_vec(const int64_t* s, int epc) { return s[0] % epc == 0 && s[1] % epc == 0 && s[2] % epc == 0; }

// compute units of the current device (persistent grids), cached per device
inline int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

}  // namespace sae

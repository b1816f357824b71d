// Shared helpers for the janus HIP library (gfx950 / CDNA4 only).
//
// Error model: every extern "C" entry point returns int (0 = OK) and never lets a
// C++ exception cross the ABI; the message is kept per thread and read back with
// janus_last_error().
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <stdexcept>
#include <type_traits>
#include "errors.h"

namespace janus {

// CUs a stream may dispatch to: the popcount of its CU mask (hipExtStreamGetCUMask; all
// CUs for an unmasked stream). Cached per stream handle. Persistent / per-CU grids size
// themselves with it, so a kernel on a half-GPU partition runs one round, not two.
int stream_cu_count(hipStream_t s);

#define JANUS_HIP(expr)                                                          \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess)                                                        \
      throw ::janus::Error(std::string(#expr) + ": " + hipGetErrorString(e_) +   \
                           " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

// Launch check after <<<>>> (launch config errors surface here, not faults).
#define JANUS_LAUNCH_CHECK() JANUS_HIP(hipGetLastError())

// The opt-in a kernel needs before it launches with more than 64 KB of dynamic LDS
// (hipFuncAttributeMaxDynamicSharedMemorySize), made once per kernel per process. The
// once-flag belongs to the instantiation, so it cannot disagree with the kernel it guards, and
// launchers that run on several host threads (one per decode lane) may arrive together.
// One flag per process, not per device: the library runs one device per process.
template <auto Kernel>
void allow_dynamic_lds(int bytes) {
  static std::once_flag once;
  std::call_once(once, [bytes] {
    JANUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  });
}

// A kernel chosen at run time travels with its opt-in: what a launcher's kernel table holds.
template <class Fn>
struct LdsKernel {
  Fn* fn;
  void (*allow)(int bytes);
};
template <auto Kernel>
constexpr LdsKernel<std::remove_pointer_t<decltype(Kernel)>> lds_kernel() {
  return {Kernel, &allow_dynamic_lds<Kernel>};
}

constexpr int kWave = 64;  // CDNA wavefront width (never 32)

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace janus

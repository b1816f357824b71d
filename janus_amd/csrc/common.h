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
#include <string>
#include <stdexcept>
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

constexpr int kWave = 64;  // CDNA wavefront width (never 32)

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace janus

// Int8 projections of the Whisper encoder on the i8 MFMA (v_mfma_i32_16x16x64_i8), the
// compute type the reference asks for (transcriber.py:23-27, compute_type='int8'), and the
// row-wise symmetric quantiser that feeds them (CTranslate2's rule, stated to the rounding
// in DESIGN.md §5j):
//   amax = max |x[k]|;  amax == 0: q = 0, scale = 1
//   else inv = 127 / amax, q[k] = clamp(rint(x[k] * inv), -127, 127), scale = amax / 127
//
//   quant_rows_kernel       fp16 (activations) or fp32 (weights) rows -> int8 rows + scale
//   layernorm_quant_kernel  norm.hip's fp32 -> fp16 LayerNorm with the quantiser applied to
//                           the fp16-rounded row in registers (the fp16 row is never stored)
//   gemm_i8_kernel          C[M,N] = epi( float(sum_k A[m,k] W[n,k]) * (sa[m] * sw[n]) + bias[n] )
//
// GEMM geometry: 128 x 128 block tile, 4 waves (2 x 2, 64 x 64 outputs each = 4 x 4 tiles
// of 16x16x64), k-tiles of 64 (one MFMA k-step) in a 3-slot LDS ring (16 KB each, two
// k-tiles in flight, counted vmcnt + raw s_barrier), 48 KB of LDS: three blocks per CU.
// Staging is gemm_big.hip's: global_load_lds (16 B per lane, no VGPR round trip), LDS rows of
// 64 B (64 int8 = 4 chunks of 16 B) XOR-swizzled on the per-lane source address and again on
// the fragment read (lane l: row l & 15, chunk l >> 4 — 16 consecutive k per lane for A and
// for B alike). The int32 accumulation
// is exact, so the result does not depend on the tiling or the k order. Rows past M are
// clamped on load and masked on store; the scale vectors are read at clamped rows / in-range
// columns only.
#include "common.h"
#include "mfma.h"
#include "kernels.h"

namespace janus {

namespace {
constexpr int kBM = 128, kBN = 128, kBK = 64;    // kBK in int8 = bytes: one MFMA k-step
constexpr int kThreads = 256;                    // 4 waves
constexpr int kWT = 4;                           // 16x16 tiles per wave and direction (64 x 64)
constexpr int kStageBytes = (kBM + kBN) * kBK;   // one ring slot (16 KB): A tile then W tile
constexpr int kSlots = 3;
constexpr int kStageDmas = 4;                    // DMA instructions per lane and k-tile
constexpr int kEP = 68;                          // epilogue pitch in 4-byte words (64 + 4)
constexpr int kEpWave = 32 * kEP;                // words per wave in the epilogue image
constexpr int kSmemBytes = 4 * kEpWave * 4 > kSlots * kStageBytes ? 4 * kEpWave * 4 : kSlots * kStageBytes;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef signed char i8x4 __attribute__((ext_vector_type(4)));
typedef signed char i8x8 __attribute__((ext_vector_type(8)));
}  // namespace

// ------------------------------------------------------------------------ quantiser
__device__ __forceinline__ float quant_inv(float amax) { return __fdiv_rn(127.0f, amax); }
__device__ __forceinline__ float quant_scale(float amax) {
  return amax == 0.0f ? 1.0f : __fdiv_rn(amax, 127.0f);
}
// amax == 0: every x is +-0, inv is unused (0 * 0)
__device__ __forceinline__ signed char quant_one(float x, float inv) {
#pragma clang fp contract(off)
  const float t = rintf(x * inv);
  return (signed char)(int)fminf(fmaxf(t, -127.0f), 127.0f);
}

__device__ __forceinline__ void load8(const _Float16* p, float (&v)[8]) {
  const half8 h = *reinterpret_cast<const half8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// One wave per row, the row in registers (8 elements per lane and step, K <= 512 * MAXV).
template <class T, int MAXV>
__global__ __launch_bounds__(256) void quant_rows_kernel(const T* __restrict__ x, int64_t ldx,
                                                         signed char* __restrict__ q, int64_t ldq,
                                                         float* __restrict__ scale, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nv = K / 8;
  const T* xr = x + (int64_t)row * ldx;
  float v[MAXV][8];
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    if (i < nv) {
      load8(xr + 8 * i, v[k]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[k][j]));
  }
  amax = wave_max_f32(amax);
  const float inv = amax == 0.0f ? 0.0f : quant_inv(amax);
  if (lane == 0) scale[row] = quant_scale(amax);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    if (i >= nv) continue;
    i8x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = quant_one(v[k][j], inv);
    *reinterpret_cast<i8x8*>(q + (int64_t)row * ldq + 8 * i) = o;
  }
}

template <class T>
static void quant_rows_dispatch(const T* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                                int K, hipStream_t s) {
  JANUS_CHECK(x && q && scale, "quant_rows_i8: null argument");
  JANUS_CHECK(K > 0 && K % 16 == 0 && K <= 3072, "quant_rows_i8: K must be a multiple of 16, <= 3072");
  JANUS_CHECK(ldx >= K && ldq >= K && ldx % 8 == 0 && ldq % 8 == 0, "quant_rows_i8: row strides");
  JANUS_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0, "quant_rows_i8: alignment");
  if (M <= 0) return;
  const int grid = (M + 3) / 4;
  signed char* qq = reinterpret_cast<signed char*>(q);
  if (K <= 512) quant_rows_kernel<T, 1><<<grid, 256, 0, s>>>(x, ldx, qq, ldq, scale, M, K);
  else if (K <= 1024) quant_rows_kernel<T, 2><<<grid, 256, 0, s>>>(x, ldx, qq, ldq, scale, M, K);
  else if (K <= 2048) quant_rows_kernel<T, 4><<<grid, 256, 0, s>>>(x, ldx, qq, ldq, scale, M, K);
  else quant_rows_kernel<T, 6><<<grid, 256, 0, s>>>(x, ldx, qq, ldq, scale, M, K);
  JANUS_LAUNCH_CHECK();
}

void quant_rows_i8_launch(const _Float16* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                          int K, hipStream_t s) {
  quant_rows_dispatch(x, ldx, q, ldq, scale, M, K, s);
}

void quant_rows_f32_i8_launch(const float* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                              int K, hipStream_t s) {
  quant_rows_dispatch(x, ldx, q, ldq, scale, M, K, s);
}

// The prepare-time weight quantiser (the decoder's int8 weights; K reaches 5120): one wave per
// fp16 row, the row read twice (amax, then q) instead of held in registers, so any K % 8 == 0.
// The arithmetic is quant_rows_kernel's, operation for operation.
__global__ __launch_bounds__(256) void quant_weight_rows_kernel(const _Float16* __restrict__ x, int64_t ldx,
                                                                signed char* __restrict__ q, int64_t ldq,
                                                                float* __restrict__ scale, int M, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nv = K / 8;
  const _Float16* xr = x + (int64_t)row * ldx;
  float v[8];
  float amax = 0.0f;
  for (int i = lane; i < nv; i += 64) {
    load8(xr + 8 * i, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
  amax = wave_max_f32(amax);
  const float inv = amax == 0.0f ? 0.0f : quant_inv(amax);
  if (lane == 0) scale[row] = quant_scale(amax);
  for (int i = lane; i < nv; i += 64) {
    load8(xr + 8 * i, v);
    i8x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = quant_one(v[j], inv);
    *reinterpret_cast<i8x8*>(q + (int64_t)row * ldq + 8 * i) = o;
  }
}

void quant_weight_rows_i8_launch(const _Float16* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                                 int K, hipStream_t s) {
  JANUS_CHECK(x && q && scale, "quant_weight_rows_i8: null argument");
  JANUS_CHECK(K > 0 && K % 8 == 0, "quant_weight_rows_i8: K must be a multiple of 8");
  JANUS_CHECK(ldx >= K && ldq >= K && ldx % 8 == 0 && ldq % 8 == 0, "quant_weight_rows_i8: row strides");
  JANUS_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 7) == 0, "quant_weight_rows_i8: alignment");
  if (M <= 0) return;
  quant_weight_rows_kernel<<<(M + 3) / 4, 256, 0, s>>>(x, ldx, reinterpret_cast<signed char*>(q), ldq, scale, M, K);
  JANUS_LAUNCH_CHECK();
}

// layernorm_kernel (norm.hip) statement for statement up to the fp16 row, which stays in
// registers and goes through the quantiser: bit-identical, q and scale, to layernorm_launch
// followed by quant_rows_i8_launch.
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_quant_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ b,
                                                              signed char* __restrict__ qout,
                                                              float* __restrict__ scale, int rows,
                                                              int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = d / 4;
  const float4* xr = reinterpret_cast<const float4*>(x + (int64_t)row * d);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4 gg[MAXV], bb[MAXV];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    gg[k] = i < nv ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    bb[k] = i < nv ? b4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float4 v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    v[k] = i < nv ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    s += ln_sum4(v[k]);
  }
  s = wave_sum_f32(s);
  const float mean = s / d;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    if (i < nv) q += ln_sq4(v[k], mean);
  }
  q = wave_sum_f32(q);
  const float rstd = rsqrtf(q / d + eps);
  half4 h[MAXV];
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    if (i < nv) {
      h[k] = ln_norm4(v[k], mean, rstd, gg[k], bb[k]);
    } else {
      h[k] = half4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fabsf((float)h[k][j]));
  }
  amax = wave_max_f32(amax);
  const float inv = amax == 0.0f ? 0.0f : quant_inv(amax);
  if (lane == 0) scale[row] = quant_scale(amax);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + k * 64;
    if (i >= nv) continue;
    i8x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = quant_one((float)h[k][j], inv);
    *reinterpret_cast<i8x4*>(qout + (int64_t)row * d + 4 * i) = o;
  }
}

void layernorm_quant_i8_launch(const float* x, const float* g, const float* b, int8_t* q, float* scale,
                               int rows, int d, float eps, hipStream_t s) {
  JANUS_CHECK(x && g && b && q && scale, "layernorm_quant_i8: null argument");
  JANUS_CHECK(d > 0 && d % 16 == 0 && d <= 2048, "layernorm_quant_i8: d must be a multiple of 16, <= 2048");
  if (rows <= 0) return;
  const int grid = (rows + 3) / 4;
  signed char* qq = reinterpret_cast<signed char*>(q);
  if (d <= 256) layernorm_quant_kernel<1><<<grid, 256, 0, s>>>(x, g, b, qq, scale, rows, d, eps);
  else if (d <= 512) layernorm_quant_kernel<2><<<grid, 256, 0, s>>>(x, g, b, qq, scale, rows, d, eps);
  else if (d <= 1024) layernorm_quant_kernel<4><<<grid, 256, 0, s>>>(x, g, b, qq, scale, rows, d, eps);
  else layernorm_quant_kernel<8><<<grid, 256, 0, s>>>(x, g, b, qq, scale, rows, d, eps);
  JANUS_LAUNCH_CHECK();
}

// ----------------------------------------------------------------------------- GEMM
// LDS rows are 64 B (4 chunks of 16 B); chunk c of row r sits at c ^ g[(r >> 2) & 3],
// g = {0, 2, 3, 1} (gemm_big.hip's 64-B-row swizzle): the ds_read_b128 lane groups of the
// fragment reads (rows lane & 15, chunk lane >> 4) cover 16 distinct 16-B bank slots.
__device__ __forceinline__ int sw64_i8(int r) { return (0x1320 >> (4 * ((r >> 2) & 3))) & 3; }

// DMA one 16-row x 64-B piece per wave-instruction: lane l -> row (l >> 2) of the piece,
// physical chunk l & 3 holding logical chunk (l & 3) ^ g[(row >> 2) & 3]
__device__ __forceinline__ void glds_rows16_i8(const signed char* __restrict__ src, int64_t ld,
                                               int row_g, int row_l, int max_row, int k0,
                                               signed char* lds_piece, int lane) {
  const int r = row_l + (lane >> 2);
  const int c = (lane & 3) ^ sw64_i8(r);
  const int gr = min(row_g + (lane >> 2), max_row);
  const signed char* g = src + (int64_t)gr * ld + k0 + 16 * c;
  typedef __attribute__((address_space(3))) void lds_void;
  __builtin_amdgcn_global_load_lds((const void*)g, (lds_void*)lds_piece, 16, 0, 0);
}

// this wave's DMAs but the newest N_ have landed and its fragment reads retired, then the
// block barrier
template <int N_>
__device__ __forceinline__ void vm_wait_barrier_i8() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N_) : "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The epilogue's fixed arithmetic: every operation rounded once. __fmul_rn / __fadd_rn are
// plain operators to the compiler, which would contract them into an fma.
__device__ __forceinline__ float dequant_bias(int acc, float sa, float sw, float bias) {
#pragma clang fp contract(off)
  const float s = sa * sw;
  const float t = (float)acc * s;
  return t + bias;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int EPI>
__global__ __launch_bounds__(kThreads, 3) void gemm_i8_kernel(GemmI8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[kSmemBytes];
  signed char* smem = reinterpret_cast<signed char*>(smem_raw);

  const int M = p.M, N = p.N, K = p.K;
  const int nbn = N / kBN, nbm = (M + kBM - 1) / kBM;
  const int bid = xcd_remap(blockIdx.x, nbm * nbn);
  const int bm = bid / nbn, bn = bid % nbn;
  const int row0 = bm * kBM, col0 = bn * kBN;
  const int lane = threadIdx.x & 63, wid = wave_id();
  const int wm = wid >> 1, wn = wid & 1;

  // stage k-tile kt into ring slot `slot`: wave w DMAs rows [32w, 32w + 32) of the A tile and
  // of the W tile, two 16-row pieces each (kStageDmas DMA instructions per lane)
  auto stage = [&](int kt, int slot) {
    signed char* sA = smem + slot * kStageBytes;
    signed char* sB = sA + kBM * kBK;
    const int k0 = kt * kBK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rl = wid * 32 + i * 16;
      glds_rows16_i8(p.A, p.lda, row0 + rl, rl, M - 1, k0, sA + rl * kBK, lane);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rl = wid * 32 + i * 16;
      glds_rows16_i8(p.W, p.ldw, col0 + rl, rl, N - 1, k0, sB + rl * kBK, lane);
    }
  };

  i32x4 acc[kWT][kWT];
#pragma unroll
  for (int m = 0; m < kWT; ++m)
#pragma unroll
    for (int n = 0; n < kWT; ++n) acc[m][n] = i32x4{0, 0, 0, 0};

  // per-lane fragment offsets (bytes): row lane & 15 of each 16-row tile, swizzled chunk
  const int fr = lane & 15;
  const int ch = ((lane >> 4) ^ sw64_i8(fr)) * 16;
  const int a_off = (wm * 64 + fr) * kBK + ch, b_off = kBM * kBK + (wn * 64 + fr) * kBK + ch;

  const int nk = K / kBK;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int slot = 0, slot2 = 2;   // slot of k-tile kt, of kt + 2
  for (int kt = 0; kt < nk; ++kt) {
    // k-tile kt landed for every wave, and every wave is done reading k-tile kt - 1 (the
    // slot k-tile kt + 2 goes to)
    if (kt + 1 < nk) vm_wait_barrier_i8<kStageDmas>(); else vm_wait_barrier_i8<0>();
    if (kt + 2 < nk) stage(kt + 2, slot2);
    const signed char* buf = smem + slot * kStageBytes;
    i32x4 a[kWT], b[kWT];
#pragma unroll
    for (int n = 0; n < kWT; ++n) b[n] = *reinterpret_cast<const i32x4*>(buf + b_off + n * 16 * kBK);
#pragma unroll
    for (int m = 0; m < kWT; ++m) a[m] = *reinterpret_cast<const i32x4*>(buf + a_off + m * 16 * kBK);
#pragma unroll
    for (int m = 0; m < kWT; ++m)
#pragma unroll
      for (int n = 0; n < kWT; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b[n], acc[m][n], 0, 0, 0);
    slot = slot == 2 ? 0 : slot + 1;
    slot2 = slot2 == 2 ? 0 : slot2 + 1;
  }
  vm_wait_barrier_i8<0>();   // every wave's last fragment reads retired: the ring is free

  // epilogue: the wave's 64 x 64 accumulators in two passes of 32 rows through its own LDS
  // image (32 x kEP words), then 8 consecutive columns per lane: scales, bias, GELU or
  // residual in fp32 with one rounding per operation, 16-B stores.
  int* sC = reinterpret_cast<int*>(smem_raw) + wid * kEpWave;
  const int cbase = col0 + wn * 64;
  const int er = lane >> 3, ec = (lane & 7) * 8;
  const int gcol = cbase + ec;
  float bias[8], wsc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bias[j] = p.bias ? p.bias[gcol + j] : 0.0f;
    wsc[j] = p.w_scale[gcol + j];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int rbase = row0 + wm * 64 + h * 32;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < kWT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sC[(m * 16 + (lane >> 4) * 4 + r) * kEP + n * 16 + fr] = acc[2 * h + m][n][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's stores land before its reads
    __builtin_amdgcn_wave_barrier();
    // RESID: the pass's residual rows are loaded before any of its stores (R may alias C;
    // each element is read and written by the same lane)
    float4 res[4][2];
    if constexpr (EPI == EPI_RESID_F32) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int row = min(rbase + it * 8 + er, M - 1);
        res[it][0] = *reinterpret_cast<const float4*>(p.R + (int64_t)row * p.ldr + gcol);
        res[it][1] = *reinterpret_cast<const float4*>(p.R + (int64_t)row * p.ldr + gcol + 4);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int lr = it * 8 + er;
      const int row = rbase + lr;
      const float asc = p.a_scale[min(row, M - 1)];
      const i32x4 lo = *reinterpret_cast<const i32x4*>(sC + lr * kEP + ec);
      const i32x4 hi = *reinterpret_cast<const i32x4*>(sC + lr * kEP + ec + 4);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = dequant_bias(j < 4 ? lo[j] : hi[j - 4], asc, wsc[j], bias[j]);
      if (row < M) {
        if constexpr (EPI == EPI_F16 || EPI == EPI_GELU_F16) {
          half8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (_Float16)(EPI == EPI_GELU_F16 ? gelu_erf(v[j]) : v[j]);
          *reinterpret_cast<half8*>(static_cast<_Float16*>(p.C) + (int64_t)row * p.ldc + gcol) = o;
        } else {
          float* c = static_cast<float*>(p.C) + (int64_t)row * p.ldc + gcol;
          if constexpr (EPI == EPI_RESID_F32) {
            v[0] = add_rn(res[it][0].x, v[0]); v[1] = add_rn(res[it][0].y, v[1]);
            v[2] = add_rn(res[it][0].z, v[2]); v[3] = add_rn(res[it][0].w, v[3]);
            v[4] = add_rn(res[it][1].x, v[4]); v[5] = add_rn(res[it][1].y, v[5]);
            v[6] = add_rn(res[it][1].z, v[6]); v[7] = add_rn(res[it][1].w, v[7]);
          }
          *reinterpret_cast<float4*>(c) = make_float4(v[0], v[1], v[2], v[3]);
          *reinterpret_cast<float4*>(c + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();       // the next pass overwrites the image
  }
}

void gemm_i8_launch(int epi, const GemmI8Args& p, hipStream_t s) {
  JANUS_CHECK(epi == EPI_F16 || epi == EPI_GELU_F16 || epi == EPI_RESID_F32 || epi == EPI_F32,
              "gemm_i8: unsupported epilogue");
  JANUS_CHECK(p.A && p.W && p.a_scale && p.w_scale && p.C, "gemm_i8: null argument");
  JANUS_CHECK(p.M > 0 && p.N > 0 && p.K > 0, "gemm_i8: empty product");
  JANUS_CHECK(p.N % 128 == 0 && p.K % 128 == 0, "gemm_i8: N and K must be multiples of 128");
  JANUS_CHECK(p.lda >= p.K && p.ldw >= p.K && p.lda % 16 == 0 && p.ldw % 16 == 0 && p.ldc >= p.N &&
                  p.ldc % 8 == 0,
              "gemm_i8: row strides");
  JANUS_CHECK(((uintptr_t)p.A & 15) == 0 && ((uintptr_t)p.W & 15) == 0 && ((uintptr_t)p.C & 15) == 0,
              "gemm_i8: operands must be 16-byte aligned");
  if (epi == EPI_RESID_F32)
    JANUS_CHECK(p.R && p.ldr >= p.N && p.ldr % 4 == 0 && ((uintptr_t)p.R & 15) == 0, "gemm_i8: residual");
  const int64_t nb = cdiv(p.M, kBM) * (p.N / kBN);
  JANUS_CHECK(nb < (1ll << 31), "gemm_i8: too many tiles");
  const unsigned blocks = (unsigned)nb;
  switch (epi) {
    case EPI_F16: gemm_i8_kernel<EPI_F16><<<blocks, kThreads, 0, s>>>(p); break;
    case EPI_GELU_F16: gemm_i8_kernel<EPI_GELU_F16><<<blocks, kThreads, 0, s>>>(p); break;
    case EPI_RESID_F32: gemm_i8_kernel<EPI_RESID_F32><<<blocks, kThreads, 0, s>>>(p); break;
    default: gemm_i8_kernel<EPI_F32><<<blocks, kThreads, 0, s>>>(p); break;
  }
  JANUS_LAUNCH_CHECK();
}

}  // namespace janus

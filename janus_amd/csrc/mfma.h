// MFMA fragment helpers for gfx950 (CDNA4): v_mfma_f32_16x16x32_f16.
//
// Lane maps (cdna_hip_programming.md §3): lane l holds A[row l&15][k 8(l>>4)+j] and
// B[k 8(l>>4)+j][col l&15], j = 0..7 (16 B per lane); C/D: col l&15,
// row 4(l>>4)+r, r = 0..3.
#pragma once
#include "common.h"

namespace janus {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(const half8& a, const half8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below the fp16 rounding of
// every consumer): branchless, one v_rcp and one v_exp, where the library erff's
// piecewise polynomial diverges within a wave. The encoder's fc1 epilogue evaluates it
// on 2048 columns of every row.
__device__ __forceinline__ float erf_fast(float x) {
  const float a = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, a, 1.0f));
  float y = fmaf(1.061405429f, t, -1.453152027f);
  y = fmaf(y, t, 1.421413741f);
  y = fmaf(y, t, -0.284496736f);
  y = fmaf(y, t, 0.254829592f);
  y *= t;
  const float e = __builtin_amdgcn_exp2f(-a * a * 1.4426950408889634f);
  return copysignf(fmaf(-y, e, 1.0f), x);
}

__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erf_fast(x * 0.70710678118654752f));
}

// __shfl_xor(v, O) over a full wave without the LDS crossbar: the partner lane's value,
// bit for bit, so every butterfly reduction keeps its association. O = 1, 2: quad_perm;
// 8: row_ror:8; 4: row_shl:4 / row_shr:4 and a select; 16, 32: v_permlane16_swap /
// v_permlane32_swap (gfx950) and a select. Each is a few VALU cycles where a ds_bpermute
// is an LDS round trip, and reductions chain six of them (a softmax's max and sum, a
// LayerNorm's two moments). All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int O>
__device__ __forceinline__ float xshfl(float v) {
  static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "xor offset");
  const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if constexpr (O == 1) return dpp_f32<0xB1>(v);        // quad_perm [1, 0, 3, 2]
  else if constexpr (O == 2) return dpp_f32<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  else if constexpr (O == 8) return dpp_f32<0x128>(v);  // row_ror:8
  else if constexpr (O == 4) {
    const float up = dpp_f32<0x104>(v), dn = dpp_f32<0x114>(v);  // row_shl:4 / row_shr:4
    return (lane & 4) ? dn : up;
  } else if constexpr (O == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v),
                                                    __builtin_bit_cast(unsigned, v), false, false);
    return __builtin_bit_cast(float, (unsigned)((lane & 16) ? r[0] : r[1]));
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v),
                                                    __builtin_bit_cast(unsigned, v), false, false);
    return __builtin_bit_cast(float, (unsigned)((lane & 32) ? r[0] : r[1]));
  }
}
// Wave priority of the decoder's kernels: the YIN blocks that share the decoder's CUs keep
// priority 0, so the latency-bound decoder phases win the issue arbitration on a shared
// SIMD and YIN takes the cycles they leave (decoder side -4 to -5 ms per step at the same
// YIN share; with a sixth packet of vocoder work moved to it, 241.4-241.7 vs 243.6-244.0 ms
// per step, profiles/r05_dec_prio_ab.txt).
__device__ __forceinline__ void dec_wave_prio() { __builtin_amdgcn_s_setprio(3); }

template <int O>
__device__ __forceinline__ int xshfl_i(int v) {
  return __builtin_bit_cast(int, xshfl<O>(__builtin_bit_cast(float, v)));  // moves only: bits kept
}
// butterfly sum / max over the whole wave (the __shfl_xor 32, 16, ..., 1 order)
__device__ __forceinline__ float wave_sum_f32(float v) {
  v += xshfl<32>(v); v += xshfl<16>(v); v += xshfl<8>(v);
  v += xshfl<4>(v); v += xshfl<2>(v); v += xshfl<1>(v);
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
  v = fmaxf(v, xshfl<32>(v)); v = fmaxf(v, xshfl<16>(v)); v = fmaxf(v, xshfl<8>(v));
  v = fmaxf(v, xshfl<4>(v)); v = fmaxf(v, xshfl<2>(v)); v = fmaxf(v, xshfl<1>(v));
  return v;
}

// x * sigmoid(x) with the hardware reciprocal (v_rcp_f32, 1 ulp) instead of the
// ~10-instruction IEEE division: SiLU runs on every staged vocoder activation.
__device__ __forceinline__ float silu(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}

// SiLU of 8 staged fp16 activations: each through fp32 (silu above) and rounded once (fp16
// arithmetic, v_exp_f16 / v_rcp_f16, costs a few fp16 ulps instead of half of one).
__device__ __forceinline__ half8 silu_h8(half8 v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (_Float16)silu((float)v[j]);
  return v;
}

// Streaming activation traffic of the vocoder (tiles read once per unit, outputs written
// once): the accesses carry the non-temporal hint, so the multi-GB vocoder stream does not
// displace what the concurrently running decoder re-reads (encoder output, weights) from
// the caches.
// Measured (overlapped bench step, r02): non-temporal OUTPUT stores — 324.3 -> 319.3 ms,
// both sides faster (decoder -5.5 ms: its re-read encoder output and weights survive in
// the caches; vocoder -3 ms); non-temporal loads as well then cost the vocoder +4.5 ms
// (the tile's halo / residual re-reads missed) for a -3 ms decoder. r03 v3: with the wide
// units' residual resident and the vocoder side ~11 ms shorter than the decoder's, every
// activation access is non-temporal by default: decoder side 278.4 -> 275.7 ms, vocoder
// side +2 ms, step 289.6-290.7 -> 287.2-287.9 ms (A/B on one box; the staging loads alone
// change nothing, the gain is the residual / accumulator re-reads).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_nt(const _Float16* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 ld_act(const _Float16* p) { return ld_nt(p); }  // tile staging
// Tile staging of the C = 64 / 32 units, `keep`: the row is loaded with the default policy
// and stays in L2, where the neighbouring tile (same XCD: xcd_remap) finds the halo rows it
// re-reads and this tile's epilogue the body rows it re-reads as the residual; else
// non-temporal. Keeping every staged row (r04, staggered step): traffic 1.26 / 1.36x ->
// 1.00 / 1.00x of the algorithmic bytes, step level-to-better in two same-box pairs (266.2 /
// 266.9 vs 266.6 / 267.7 ms) against keeping only the halo rows (r04 v2).
__device__ __forceinline__ uint4 ld_act_halo(const _Float16* p, bool keep) {
  if (keep) return *reinterpret_cast<const uint4*>(p);
  return ld_nt(p);
}
__device__ __forceinline__ uint4 ld_res(const _Float16* p) { return ld_nt(p); }  // epilogue re-reads
__device__ __forceinline__ void st_act(_Float16* p, const half8& v) {
  __builtin_nontemporal_store(v, reinterpret_cast<half8*>(p));
}

// 8 int8 weights -> 8 fp16, exact (every int8 value is an fp16): the bytes with their sign
// bit flipped (q + 128 in 0 .. 255) are permuted under the exponent byte 0x64, which reads as
// the fp16 1024 + (q + 128) (ulp 1 in [1024, 2048)), and one packed subtract of 1152 leaves q.
// 4 v_perm_b32 + 2 v_xor + 4 v_pk_add_f16 per 8 weights. Element j is byte j.
__device__ __forceinline__ half8 w8_half8(uint2 q) {
  const unsigned lo = q.x ^ 0x80808080u, hi = q.y ^ 0x80808080u;
  constexpr unsigned ex = 0x64646464u;  // selector bytes 0-3: the weights' bytes, 4-7: ex's
  const u32x4 u = {__builtin_amdgcn_perm(ex, lo, 0x04010400u), __builtin_amdgcn_perm(ex, lo, 0x04030402u),
                   __builtin_amdgcn_perm(ex, hi, 0x04010400u), __builtin_amdgcn_perm(ex, hi, 0x04030402u)};
  half8 off;
#pragma unroll
  for (int j = 0; j < 8; ++j) off[j] = (_Float16)1152.0f;
  return __builtin_bit_cast(half8, u) - off;
}

__device__ __forceinline__ half8 zero_half8() {
  half8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (_Float16)0.0f;
  return z;
}

// Wave index within the block as a wave-uniform (SGPR) value: tid >> 6 alone is a VGPR
// to the compiler, so branches on it (m-tile / head ownership) became exec-masked
// branches with accumulators shuttled through VGPRs around every MFMA.
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

__device__ __forceinline__ f32x4 zero_f32x4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// LDS row pitch (in halves) for tiles read as MFMA fragments with ds_read_b128: a pitch
// of 16*P bytes with P % 4 == 2 puts the 16 lanes of every gfx950 b128 lane group
// ({0-3,12-15,20-27}, ...: rows r, r+12.. of one 16-B column chunk and rows r+4.. of the
// next) on 16 distinct 4-bank slots — conflict-free. (P % 4 == 1, e.g. the classic
// "+8 halves" pad of a 64-half row, is 2-way.)
__host__ __device__ constexpr int frag_pitch(int min_halves) {
  int p = (min_halves + 7) / 8;
  while (p % 4 != 2) ++p;
  return p * 8;
}

// XCD-aware remap of a 1-D block index (bijective; MI355X deals blocks round-robin
// over 8 XCDs, so consecutive logical tiles are placed on one XCD's L2).
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
  constexpr int kXcd = 8;
  if (nblocks < kXcd) return bid;
  const int q = nblocks / kXcd, r = nblocks % kXcd;
  const int xcd = bid % kXcd, idx = bid / kXcd;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// The vocoder kernels take their tiles in this order: against plain dispatch order the
// standalone vocoder's L2->fabric traffic fell from 1.42x to 1.19x the algorithmic bytes
// (profiles/traffic_r02.json).

// Store an MFMA output fragment (lane = column col = tile column (lane & 15), rows row0 + rr,
// rr < 4, row0 = m*16 + 4*(lane >> 4)) as fp16 into an LDS tile, one 2-byte store per
// element. Trading halves with lane l^1 (one DPP move) for 4-byte stores measured slower
// (standalone 64 x 30 s vocoder 154.0 vs 151.9 ms), so the LDS bank conflicts of the wide
// units do not come from these stores.
__device__ __forceinline__ void st_frag_f16(_Float16* tile, int ld, int row0, int col, const float (&v)[4]) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) tile[(row0 + rr) * ld + col] = (_Float16)v[rr];
}

// LayerNorm arithmetic shared by layernorm_kernel and resid_ln_kernel (gemm.hip), written
// with explicit fmaf and no other contraction so the two kernels round alike: left to the
// compiler, a*a + b*b may become fma(a, a, b*b) in one kernel and fma(b, b, a*a) in the
// other.
__device__ __forceinline__ float ln_sum4(const float4& v) {
#pragma clang fp contract(off)
  return ((v.x + v.y) + v.z) + v.w;
}
__device__ __forceinline__ float ln_sq4(const float4& v, float mean) {
#pragma clang fp contract(off)
  const float a = v.x - mean, b = v.y - mean, c = v.z - mean, e = v.w - mean;
  return fmaf(e, e, fmaf(c, c, fmaf(b, b, a * a)));
}
__device__ __forceinline__ half4 ln_norm4(const float4& v, float mean, float rstd, const float4& g,
                                          const float4& b) {
#pragma clang fp contract(off)
  return half4{(_Float16)fmaf((v.x - mean) * rstd, g.x, b.x), (_Float16)fmaf((v.y - mean) * rstd, g.y, b.y),
               (_Float16)fmaf((v.z - mean) * rstd, g.z, b.z), (_Float16)fmaf((v.w - mean) * rstd, g.w, b.w)};
}

// LayerNorm of R fp32 rows by one wave (rows row0 + j*rstep, j < R; d <= 256*MAXV, d % 4
// == 0): every row, gamma and beta load is issued before the first use (one memory round
// trip for all R rows); fp16 out rows at out + (lrow0 + j*rstep)*ldo, ALL R of them written
// (rows >= nrows as zeros: out must hold R rows, e.g. an LDS tile).
// Two-pass mean / variance in fp32 as layernorm_kernel. MAXV sized to d keeps the register
// footprint small enough not to cost the caller occupancy; the loads are unconditional
// (clamped index) — guarded vector loads are split into branchy dword loads by the
// compiler, which measured 3x slower in the GEMM prologue.
template <int MAXV, int R>
__device__ __forceinline__ void ln_rows_wave(const float* x, int64_t ldx, int row0, int rstep,
                                             int nrows, const float* __restrict__ g,
                                             const float* __restrict__ b, _Float16* out,
                                             int lrow0, int ldo, int d, float eps, int lane) {
  const int nv = d >> 2;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4 v[R][MAXV], gg[MAXV], bb[MAXV];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int r = row0 + j * rstep;
    const float4* x4 = reinterpret_cast<const float4*>(x + (int64_t)min(r, nrows - 1) * ldx);
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int i = lane + 64 * k;
      // unconditional 16-byte loads (clamped index; values past d are masked below)
      v[j][k] = x4[min(i, nv - 1)];
    }
  }
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = min(lane + 64 * k, nv - 1);
    gg[k] = g4[i];
    bb[k] = b4[i];
  }
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
      if (lane + 64 * k >= nv) v[j][k] = z;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    // layernorm_kernel's arithmetic (ln_sum4 / ln_sq4 / ln_norm4): a LayerNorm in a GEMM
    // prologue rounds exactly as the separate LayerNorm launch it replaces
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) s += ln_sum4(v[j][k]);
    s = wave_sum_f32(s);
    const float mean = s / d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
      if (lane + 64 * k < nv) q += ln_sq4(v[j][k], mean);
    q = wave_sum_f32(q);
    const float rstd = rsqrtf(q / d + eps);
    const bool rok = row0 + j * rstep < nrows;
    _Float16* orow = out + (int64_t)(lrow0 + j * rstep) * ldo;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int i = lane + 64 * k;
      if (i < nv) {
        half4 h = ln_norm4(v[j][k], mean, rstd, gg[k], bb[k]);
        if (!rok) h = half4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        *reinterpret_cast<half4*>(orow + 4 * i) = h;
      }
    }
  }
}

// LayerNorm of one fp32 row of d <= 1024 columns by one wave (two-pass mean / variance
// in fp32, as layernorm_kernel), fp16 out. SC1: read the row with agent-scope relaxed
// (sc1) loads — for rows other workgroups of the same launch have just stored sc1.
template <bool SC1>
__device__ __forceinline__ void ln_row_wave(const float* xr, const float* __restrict__ g,
                                            const float* __restrict__ b, _Float16* out, int d,
                                            float eps, int lane) {
  if constexpr (SC1) {
    float v[16];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      const float t = c < d ? __hip_atomic_load(xr + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
      v[i] = t;
      s += t;
    }
    s = wave_sum_f32(s);
    const float mean = s / d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      if (c < d) q += (v[i] - mean) * (v[i] - mean);
    }
    q = wave_sum_f32(q);
    const float rstd = rsqrtf(q / d + eps);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = lane + 64 * i;
      if (c < d) out[c] = (_Float16)((v[i] - mean) * rstd * g[c] + b[c]);
    }
  } else {
    ln_rows_wave<4, 1>(xr, 0, 0, 1, 1, g, b, out, 0, 0, d, eps, lane);
  }
}

}  // namespace janus

// Band-limited polyphase resampling on gfx950 as one banded GEMM (the rule: include/janus.h).
// G periods of a rate pair are one row: Lg = G L outputs drawn from consecutive inputs, so
//   Y[row][n] = sum_k X[row Mg + k] H[k][n],
// A = the staged input itself viewed with row stride Mg (rows overlap), H = the banded tap
// matrix of the plan (resample_plan.h: per 16-column tile only the k range that holds taps).
// It runs on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain per output,
// no wider accumulation), so an output's bits depend on its phase and its inputs alone,
// not on its row in a tile, its clip or the call it came in.
//
//   resample_stage_kernel  copies clip c to its place in the staging buffer (zeroed before).
//   resample_kernel        grid (row blocks of the longest clip, clips), 4 waves, each wave
//                          2 x 16 rows; per column tile it walks the tile's k steps: B from
//                          the packed table (one coalesced 256 B load per step), A straight
//                          from the staging buffer (16 rows x 16 B per step, served by L1 /
//                          L2: the rows of a tile overlap or adjoin). No LDS.
// Every read stays inside the staging buffer by construction (audioapi.cpp sizes a clip's
// span to whole 16-row tiles plus the widest k range; a wave whose second row tile lies past
// the clip's rows re-reads its first and stores nothing for it).
#include "mfma.h"
#include "kernels.h"

namespace janus {

__global__ __launch_bounds__(256) void resample_stage_kernel(const float* __restrict__ pcm,
                                                             const int64_t* __restrict__ meta,
                                                             int n_clips, float* __restrict__ stage) {
  const int c = blockIdx.y;
  const int64_t src = meta[c], n = meta[n_clips + c], dst = meta[2 * n_clips + c];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    stage[dst + i] = pcm[src + i];
}

// meta: int64 [5][n_clips] = source offset | n_in | staging index of sample 0 | output offset | n_out
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ stage,
                                                       const int64_t* __restrict__ meta, int n_clips,
                                                       const int32_t* __restrict__ tile_meta,
                                                       const float* __restrict__ table, int Lg, int Mg,
                                                       int n_ct, float* __restrict__ out) {
  const int c = blockIdx.y, lane = threadIdx.x & 63, w = wave_id();
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t n_out = meta[4 * n_clips + c];
  const int64_t rows = (n_out + Lg - 1) / Lg;
  const int64_t row0 = ((int64_t)blockIdx.x * kResampleWaves + w) * (16 * kResampleRowTiles);
  if (row0 >= rows) return;  // wave-uniform; the kernel has no barrier
  const float* x = stage + meta[2 * n_clips + c];
  float* y = out + meta[3 * n_clips + c];
  bool ok[kResampleRowTiles];
  const float* xa[kResampleRowTiles];
#pragma unroll
  for (int m = 0; m < kResampleRowTiles; ++m) {
    ok[m] = row0 + 16 * m < rows;
    xa[m] = x + (row0 + (ok[m] ? 16 * m : 0) + l15) * Mg + l4;
  }
  for (int j = 0; j < n_ct; ++j) {
    const int kstart = tile_meta[3 * j], ksteps = tile_meta[3 * j + 1];
    const float* b = table + tile_meta[3 * j + 2] + lane;
    f32x4 acc[kResampleRowTiles];
#pragma unroll
    for (int m = 0; m < kResampleRowTiles; ++m) acc[m] = zero_f32x4();
    for (int kk = 0; kk < ksteps; ++kk) {
      const float bv = b[(int64_t)kk * 64];
#pragma unroll
      for (int m = 0; m < kResampleRowTiles; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[m][kstart + 4 * kk], bv, acc[m], 0, 0, 0);
    }
    const int col = 16 * j + l15;
    if (col < Lg) {
#pragma unroll
      for (int m = 0; m < kResampleRowTiles; ++m) {
        if (!ok[m]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t idx = (row0 + 16 * m + 4 * l4 + r) * Lg + col;
          if (idx < n_out) y[idx] = acc[m][r];
        }
      }
    }
  }
}

void resample_launch(const float* pcm, const int64_t* meta_dev, int n_clips, int64_t max_n_in,
                     int64_t max_n_out, float* stage, const int32_t* tile_meta, const float* table,
                     int Lg, int Mg, int n_ct, float* out, hipStream_t s) {
  JANUS_CHECK(n_clips <= 65535, "resample: at most 65535 clips per call");
  if (n_clips <= 0 || max_n_in <= 0) return;
  const int64_t sb = std::min<int64_t>(cdiv(max_n_in, 256), 1024);
  resample_stage_kernel<<<dim3((unsigned)sb, n_clips), 256, 0, s>>>(pcm, meta_dev, n_clips, stage);
  JANUS_LAUNCH_CHECK();
  const int64_t rb = cdiv(cdiv(max_n_out, Lg), kResampleBlockRows);
  JANUS_CHECK(rb <= 0x7fffffff, "resample: clip too long for one launch");
  resample_kernel<<<dim3((unsigned)rb, n_clips), 256, 0, s>>>(stage, meta_dev, n_clips, tile_meta, table,
                                                              Lg, Mg, n_ct, out);
  JANUS_LAUNCH_CHECK();
}

}  // namespace janus

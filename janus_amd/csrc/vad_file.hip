// Whole-file silero-vad v5 (16 kHz) on gfx950: the graph of vad.hip split where its data
// dependence splits. Only the LSTM recurrence is sequential; in a file the 64-sample
// context of chunk j is the last 64 samples of chunk j - 1, which lie in the buffer, so
// everything up to the input half of the gates depends on the audio alone.
//
//   vad_encode_kernel  parallel over (stream, tile of 16 chunks), 256 threads. Per chunk:
//                      STFT 4 x 258 x 256, conv 4 x 128 x 387, 2 x 64 x 384, 64 x 192,
//                      128 x 64 (the one tap that meets data), W_ih 512 x 128: ~0.59 M MAC,
//                      all on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf
//                      chain per output, so a chunk's result does not depend on its row in
//                      the tile). Intermediates of the tile in LDS, weights from L2.
//                      Writes pre[s][j][512] = W_ih e3 + b_ih + b_hh.
//   vad_scan_kernel    one 512-thread block per stream, thread = one row of W_hh held in
//                      128 VGPRs for the whole scan; per step 128 fmaf per thread on h
//                      broadcast from LDS, the four gates of a unit meet inside a wave
//                      (bpermute), one __syncthreads per step (h double-buffered).
//                      h_j is stored over pre[s][j][0..127].
//   vad_prob_kernel    one wave per chunk: sigm(bo + wo . relu(h_j)), vad.hip's summation
//                      order.
// fp32 throughout. Audio of S streams concatenated, offsets [S + 1]; stream s of L samples
// has L / 512 + 1 chunks, a sample index >= L (or < 0: the first context) reads as 0.
#include "mfma.h"
#include "kernels.h"

namespace janus {

constexpr int kCT = 16;                        // chunks per encoder block
constexpr int kWinRows = (kCT * 512 + 64 + 127) / 128;  // 65 rows of 128 samples
constexpr int kWinPitch = 132;                 // 16 frames x 4 k on distinct banks
constexpr int kMagPitch = 129;                 // [chunk][frame + 1 (0, 5: zero)][bin]
constexpr int kE0Pitch = 129;                  // [chunk][frame + 1 (0: zero)][channel]
constexpr int kE1Pitch = 68;                   // [chunk][frame + 1 (0: zero)][channel]
constexpr int kE2Pitch = 68, kE3Pitch = 132;   // [chunk][channel]
constexpr int kR0 = kCT * 6 * kMagPitch;       // window | mag | e0 | e2
constexpr int kR1 = kCT * 3 * kE1Pitch;        // e1 | e3
static_assert(kWinRows * kWinPitch <= kR0 && kCT * 5 * kE0Pitch <= kR0 && kCT * kE2Pitch <= kR0, "R0");
static_assert(kCT * kE3Pitch <= kR1, "R1");
static_assert((kR0 + kR1 + 128) * 4 <= 64 * 1024, "encoder LDS");

__device__ __forceinline__ f32x4 mfma_x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float sigm_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }

// LDS address of sample i of the staged window
__device__ __forceinline__ int win_at(int i) { return (i >> 7) * kWinPitch + (i & 127); }
// window index of x[128 f + k] of chunk c: x = [context | chunk | reflect pad], x[576 + t] = x[574 - t]
__device__ __forceinline__ int frame_at(int c, int f, int k) {
  return 512 * c + ((f == 3 && k >= 192) ? 766 - k : 128 * f + k);
}

__global__ __launch_bounds__(256) void vad_encode_kernel(const float* __restrict__ pcm,
                                                         const int64_t* __restrict__ offsets,
                                                         VadWeights W, int64_t pass_start,
                                                         int pass_chunks, float* __restrict__ pre) {
  __shared__ float r0[kR0];
  __shared__ float r1[kR1];
  __shared__ float nyq[128];
  const int s = blockIdx.y, t0 = blockIdx.x * kCT;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int l15 = lane & 15, l4 = lane >> 4;
  const int64_t base = offsets[s], L = offsets[s + 1] - base;
  const int64_t left = L / 512 + 1 - pass_start;            // chunks of this stream from pass_start on
  const int n_pass = (int)(left < pass_chunks ? left : pass_chunks);
  if (t0 >= n_pass) return;                                 // block-uniform
  const float* x = pcm + base;

  // ---- stage samples [512 j0 - 64, 512 (j0 + 16)) of the stream, zeros outside [0, L)
  const int64_t p0 = (pass_start + t0) * 512 - 64;
  for (int i = tid; i < kCT * 512 + 64; i += 256) {
    const int64_t p = p0 + i;
    r0[win_at(i)] = (p >= 0 && p < L) ? x[p] : 0.0f;
  }
  __syncthreads();

  // ---- STFT: rows (chunk, frame) = 64, bins 0..127 on the MFMA (wave w: bin tiles w, w + 4),
  //      bin 128 as a plain fmaf chain (waves 0, 1: real, imaginary part of the 64 rows)
  float mg[2][4][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int bin = (w + 4 * j) * 16 + l15;
    const float* br = W.basis + (int64_t)bin * 256 + l4;
    const float* bi = br + 129 * 256;
    f32x4 re[4], im[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) { re[m] = zero_f32x4(); im[m] = zero_f32x4(); }
#pragma unroll 4
    for (int kk = 0; kk < 64; ++kk) {
      const float bre = br[4 * kk], bim = bi[4 * kk];
      const int k = 4 * kk + l4;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int row = m * 16 + l15;
        const float av = r0[win_at(frame_at(row >> 2, row & 3, k))];
        re[m] = mfma_x4(av, bre, re[m]);
        im[m] = mfma_x4(av, bim, im[m]);
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) mg[j][m][r] = sqrtf(re[m][r] * re[m][r] + im[m][r] * im[m][r]);
  }
  if (w < 2) {
    const float* b = W.basis + (int64_t)(128 + 129 * w) * 256;
    const int c = lane >> 2, f = lane & 3;
    float acc = 0.f;
    for (int k = 0; k < 256; ++k) acc = fmaf(b[k], r0[win_at(frame_at(c, f, k))], acc);
    nyq[w * 64 + lane] = acc;
  }
  __syncthreads();  // every wave is done with the window: mag over it
  for (int i = tid; i < kCT * 2 * kMagPitch; i += 256) {  // frames -1 and 4 of the conv padding
    const int c = i / (2 * kMagPitch), q = i % (2 * kMagPitch);
    r0[(c * 6 + (q >= kMagPitch ? 5 : 0)) * kMagPitch + q % kMagPitch] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // accumulator row 16 m + 4 l4 + r = (chunk 4 m + l4, frame r)
        r0[((m * 4 + l4) * 6 + r + 1) * kMagPitch + (w + 4 * j) * 16 + l15] = mg[j][m][r];
  if (tid < 64) {
    const float re = nyq[tid], im = nyq[64 + tid];
    r0[((tid >> 2) * 6 + (tid & 3) + 1) * kMagPitch + 128] = sqrtf(re * re + im * im);
  }
  __syncthreads();

  // ---- conv0 129 -> 128, stride 1: rows (chunk, t) = 64, K = (ci, tap) = 387; wave w: co tiles 2w, 2w + 1
  {
    f32x4 acc[4][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const float bv = W.b0[(2 * w + n) * 16 + l15];
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[m][n] = splat4(bv);
    }
    const float* wp = W.w0 + (int64_t)(2 * w * 16 + l15) * 387;
#pragma unroll 4
    for (int kk = 0; kk < 97; ++kk) {
      const int kidx = 4 * kk + l4;
      const bool ok = kidx < 387;
      const int kc = ok ? kidx : 0;
      const float b0v = ok ? wp[kc] : 0.0f, b1v = ok ? wp[16 * 387 + kc] : 0.0f;
      const int ci = kc / 3, tap = kc % 3;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int row = m * 16 + l15;
        const float av = ok ? r0[((row >> 2) * 6 + (row & 3) + tap) * kMagPitch + ci] : 0.0f;
        acc[m][0] = mfma_x4(av, b0v, acc[m][0]);
        acc[m][1] = mfma_x4(av, b1v, acc[m][1]);
      }
    }
    __syncthreads();  // mag is read: e0 over it
    for (int i = tid; i < kCT * kE0Pitch; i += 256)
      r0[(i / kE0Pitch) * 5 * kE0Pitch + i % kE0Pitch] = 0.0f;  // frame -1
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          r0[((m * 4 + l4) * 5 + r + 1) * kE0Pitch + (2 * w + n) * 16 + l15] = fmaxf(acc[m][n][r], 0.0f);
  }
  __syncthreads();

  // ---- conv1 128 -> 64, stride 2: rows (chunk, t) = 32, K = 384; wave w: co tile w
  {
    f32x4 acc[2];
    acc[0] = acc[1] = splat4(W.b1[w * 16 + l15]);
    const float* wp = W.w1 + (int64_t)(w * 16 + l15) * 384;
#pragma unroll 4
    for (int kk = 0; kk < 96; ++kk) {
      const int kidx = 4 * kk + l4;
      const float bv = wp[kidx];
      const int ci = kidx / 3, tap = kidx % 3;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int row = m * 16 + l15;  // (chunk row >> 1, t = row & 1): input frame 2 t + tap - 1
        const float av = r0[((row >> 1) * 5 + 2 * (row & 1) + tap) * kE0Pitch + ci];
        acc[m] = mfma_x4(av, bv, acc[m]);
      }
    }
    for (int i = tid; i < kCT * kE1Pitch; i += 256)
      r1[(i / kE1Pitch) * 3 * kE1Pitch + i % kE1Pitch] = 0.0f;  // frame -1
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m * 16 + 4 * l4 + r;
        r1[((row >> 1) * 3 + (row & 1) + 1) * kE1Pitch + w * 16 + l15] = fmaxf(acc[m][r], 0.0f);
      }
  }
  __syncthreads();

  // ---- conv2 64 -> 64, stride 2, one output frame: rows = 16 chunks, K = 192; wave w: co tile w
  {
    f32x4 acc = splat4(W.b2[w * 16 + l15]);
    const float* wp = W.w2 + (int64_t)(w * 16 + l15) * 192;
#pragma unroll 4
    for (int kk = 0; kk < 48; ++kk) {
      const int kidx = 4 * kk + l4;
      const int ci = kidx / 3, tap = kidx % 3;
      acc = mfma_x4(r1[(l15 * 3 + tap) * kE1Pitch + ci], wp[kidx], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) r0[(4 * l4 + r) * kE2Pitch + w * 16 + l15] = fmaxf(acc[r], 0.0f);
  }
  __syncthreads();

  // ---- conv3 64 -> 128 on one frame: only the middle tap meets data. K = 64; wave w: co tiles 2w, 2w + 1
  {
    f32x4 acc[2];
    acc[0] = splat4(W.b3[(2 * w) * 16 + l15]);
    acc[1] = splat4(W.b3[(2 * w + 1) * 16 + l15]);
    const float* wp = W.w3 + (int64_t)(2 * w * 16 + l15) * 192 + 1;
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      const int ci = 4 * kk + l4;
      const float av = r0[l15 * kE2Pitch + ci];
      acc[0] = mfma_x4(av, wp[ci * 3], acc[0]);
      acc[1] = mfma_x4(av, wp[16 * 192 + ci * 3], acc[1]);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        r1[(4 * l4 + r) * kE3Pitch + (2 * w + n) * 16 + l15] = fmaxf(acc[n][r], 0.0f);
  }
  __syncthreads();

  // ---- input half of the gates: rows = 16 chunks, N = 512 (wave w: gate tiles 8w .. 8w + 7), K = 128
  {
    f32x4 acc[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int g = (8 * w + n) * 16 + l15;
      acc[n] = splat4(W.bih[g] + W.bhh[g]);
    }
    const float* wp = W.wih + (int64_t)(8 * w * 16 + l15) * 128 + l4;
#pragma unroll 2
    for (int kk = 0; kk < 32; ++kk) {
      const float av = r1[l15 * kE3Pitch + 4 * kk + l4];
#pragma unroll
      for (int n = 0; n < 8; ++n) acc[n] = mfma_x4(av, wp[n * 16 * 128 + 4 * kk], acc[n]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jj = t0 + 4 * l4 + r;  // chunk within the pass
      if (jj >= n_pass) continue;
      float* out = pre + ((int64_t)s * pass_chunks + jj) * 512;
#pragma unroll
      for (int n = 0; n < 8; ++n) out[(8 * w + n) * 16 + l15] = acc[n][r];
    }
  }
}

// Thread tid of wave v, lane l: unit u = 16 v + (l & 15), gate q = l >> 4 (i, f, g, o):
// row q * 128 + u of W_hh. The four gates of a unit sit in one wave.
__global__ __launch_bounds__(512) void vad_scan_kernel(float* __restrict__ pre,
                                                       const float* __restrict__ whh,
                                                       const int64_t* __restrict__ offsets,
                                                       int64_t pass_start, int pass_chunks,
                                                       float* __restrict__ hc_state) {
  __shared__ float4 hs[2][32];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int u = (tid >> 6) * 16 + (lane & 15), q = lane >> 4, g = q * 128 + u;
  const int64_t left = (offsets[s + 1] - offsets[s]) / 512 + 1 - pass_start;
  const int n = (int)(left < pass_chunks ? left : pass_chunks);
  if (n <= 0) return;  // block-uniform
  float wr[128];
  {
    const float4* w4 = reinterpret_cast<const float4*>(whh + (int64_t)g * 128);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const float4 v = w4[k];
      wr[4 * k] = v.x; wr[4 * k + 1] = v.y; wr[4 * k + 2] = v.z; wr[4 * k + 3] = v.w;
    }
  }
  float* hc = hc_state + (int64_t)s * 256;
  float c = hc[128 + u];
  if (q == 0) reinterpret_cast<float*>(hs[0])[u] = hc[u];
  float* row = pre + (int64_t)s * pass_chunks * 512;
  float pj = row[g];
  __syncthreads();
  float hn = 0.f;
  for (int j = 0; j < n; ++j) {
    const float pnext = row[(int64_t)(j + 1 < n ? j + 1 : j) * 512 + g];  // in flight during the step
    const float4* h4 = hs[j & 1];
    float a0 = pj, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const float4 h = h4[k];
      a0 = fmaf(wr[4 * k], h.x, a0);
      a1 = fmaf(wr[4 * k + 1], h.y, a1);
      a2 = fmaf(wr[4 * k + 2], h.z, a2);
      a3 = fmaf(wr[4 * k + 3], h.w, a3);
    }
    const float gate = (a0 + a1) + (a2 + a3);
    const float act = q == 2 ? tanhf(gate) : sigm_f(gate);
    const float ig = __shfl(act, lane & 15), fg = __shfl(act, 16 + (lane & 15));
    const float gg = __shfl(act, 32 + (lane & 15)), og = __shfl(act, 48 + (lane & 15));
    c = fg * c + ig * gg;
    hn = og * tanhf(c);
    if (q == 0) {
      reinterpret_cast<float*>(hs[(j + 1) & 1])[u] = hn;
      row[(int64_t)j * 512 + u] = hn;  // pre[j] was consumed a step ago: h_j for the probability
    }
    pj = pnext;
    __syncthreads();
  }
  if (q == 0) { hc[u] = hn; hc[128 + u] = c; }
}

// prob = sigm(bo + wo . relu(h_j)), summed as vad.hip sums it: units 0..63 and 64..127 by a
// wave butterfly each, then (r0 + r1) + (0 + 0).
__global__ __launch_bounds__(256) void vad_prob_kernel(const float* __restrict__ pre,
                                                       const float* __restrict__ wo,
                                                       const float* __restrict__ bo,
                                                       const int64_t* __restrict__ offsets,
                                                       const int64_t* __restrict__ chunk_off,
                                                       int64_t pass_start, int pass_chunks,
                                                       float* __restrict__ prob) {
  const int s = blockIdx.y, lane = threadIdx.x & 63;
  const int jj = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t left = (offsets[s + 1] - offsets[s]) / 512 + 1 - pass_start;
  if (jj >= pass_chunks || jj >= left) return;  // wave-uniform
  const float* h = pre + ((int64_t)s * pass_chunks + jj) * 512;
  float c0 = wo[lane] * fmaxf(h[lane], 0.0f), c1 = wo[64 + lane] * fmaxf(h[64 + lane], 0.0f);
  for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); }
  if (lane == 0) prob[chunk_off[s] + pass_start + jj] = sigm_f(bo[0] + ((c0 + c1) + (0.0f + 0.0f)));
}

void silero_vad_file_launch(const float* pcm, const int64_t* offsets_dev, const int64_t* chunk_off_dev,
                            int n_streams, int64_t max_chunks, int pass_chunks, const VadWeights& W,
                            float* pre, float* hc_state, float* prob, hipStream_t s) {
  JANUS_CHECK(n_streams <= 65535, "vad: at most 65535 streams per call");
  JANUS_CHECK(pass_chunks >= 1, "vad: a pass holds at least one chunk");
  if (n_streams <= 0) return;
  JANUS_HIP(hipMemsetAsync(hc_state, 0, sizeof(float) * 256 * n_streams, s));  // fresh model per stream
  for (int64_t start = 0; start < max_chunks; start += pass_chunks) {
    const int np = (int)std::min<int64_t>(pass_chunks, max_chunks - start);  // chunks of the longest stream
    vad_encode_kernel<<<dim3((np + kCT - 1) / kCT, n_streams), 256, 0, s>>>(pcm, offsets_dev, W, start,
                                                                            pass_chunks, pre);
    JANUS_LAUNCH_CHECK();
    vad_scan_kernel<<<n_streams, 512, 0, s>>>(pre, W.whh, offsets_dev, start, pass_chunks, hc_state);
    JANUS_LAUNCH_CHECK();
    vad_prob_kernel<<<dim3((np + 3) / 4, n_streams), 256, 0, s>>>(pre, W.wo, W.bo, offsets_dev,
                                                                  chunk_off_dev, start, pass_chunks, prob);
    JANUS_LAUNCH_CHECK();
  }
}

}  // namespace janus

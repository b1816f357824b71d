// Word-level timestamps (janus_whisper_align, include/janus.h): the kernels of the alignment
// pass. A teacher-forced decoder forward over each window's whole token sequence keeps the
// cross-attention probabilities of the alignment heads; they are normalised over the rows,
// median-filtered along the frames and averaged over the heads (align_reduce), and a
// dynamic-time-warping solve over the negated result gives the token -> frame path
// (align_dtw). The linear layers of the forward run on the existing GEMM / LayerNorm
// launchers; this file adds what a whole-sequence pass needs and the per-step decoder has
// not: attention over a tile of query rows.
#include <cmath>
#include "align.h"
#include "mfma.h"

namespace janus {

// ------------------------------------------------------------------ embedding
__global__ __launch_bounds__(256) void align_embed_kernel(const _Float16* __restrict__ tok_emb,
                                                          const float* __restrict__ pos_emb,
                                                          const int32_t* __restrict__ tok,
                                                          const int32_t* __restrict__ pos, int d,
                                                          float* __restrict__ x) {
  const int r = blockIdx.x;
  const int64_t t = tok[r], p = pos[r];
  for (int c = threadIdx.x; c < d; c += 256)
    x[(int64_t)r * d + c] = (float)tok_emb[t * d + c] + pos_emb[p * d + c];
}

void align_embed_launch(const _Float16* tok_emb, const float* pos_emb, const int32_t* tok,
                        const int32_t* pos, int M, int d, float* x, hipStream_t s) {
  if (M <= 0) return;
  align_embed_kernel<<<M, 256, 0, s>>>(tok_emb, pos_emb, tok, pos, d, x);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ attention
// Block: 4 waves, 16 query rows of one (window, head). Phase 1: the waves take the 16-key
// tiles in turn, S = Q K^T (two 16x16x32 MFMAs per tile: head_dim 64) scaled and masked into
// the fp32 row buffer sS [16][SP]. Phase 2: each wave owns 4 rows: max, exp, sum, divide —
// the probabilities stay in sS and, for an alignment head, frames < F go to global memory.
// Phase 3: wave w computes output columns 16w .. 16w + 15, P (fp16 from sS) x V over 32-key
// steps. Every load is clamped into the window's rows / keys; masked keys hold -inf.
__global__ __launch_bounds__(256) void align_attn_kernel(AlignAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sS[];
  const int tile = blockIdx.x, h = blockIdx.y;
  const int w = a.tiles[2 * tile], q0 = a.tiles[2 * tile + 1];
  const AlignWinDev W = a.wins[w];
  const bool causal = a.Tk == 0;
  const int n = W.n;
  const int Tk = causal ? min(n, q0 + kAlignTileRows) : a.Tk;
  const int64_t kbase = causal ? (int64_t)W.row0 : (int64_t)W.enc_row * a.Tk;
  const int Tp = (Tk + 31) & ~31, SP = Tp + 4;
  const int lane = threadIdx.x & 63, wid = wave_id();
  const int l15 = lane & 15, lg = lane >> 4;

  const int64_t qr = (int64_t)W.row0 + min(q0 + l15, n - 1);
  const _Float16* qp = a.q + qr * a.ldq + h * 64 + 8 * lg;
  const half8 qa0 = *reinterpret_cast<const half8*>(qp);
  const half8 qa1 = *reinterpret_cast<const half8*>(qp + 32);
  for (int kt = wid; kt < Tp / 16; kt += 4) {
    const int t = kt * 16 + l15;
    const _Float16* kp = a.k + (kbase + min(t, Tk - 1)) * a.ldkv + h * 64 + 8 * lg;
    const half8 kb0 = *reinterpret_cast<const half8*>(kp);
    const half8 kb1 = *reinterpret_cast<const half8*>(kp + 32);
    f32x4 acc = mfma16(qa0, kb0, zero_f32x4());
    acc = mfma16(qa1, kb1, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * lg + r;
      const bool ok = t < Tk && (!causal || t <= q0 + row);
      sS[row * SP + t] = ok ? acc[r] * a.scale : -INFINITY;
    }
  }
  __syncthreads();

  const int slot = a.probs ? a.slots[h] : -1;
  for (int rr = 0; rr < 4; ++rr) {
    const int row = wid * 4 + rr;
    float* sr = sS + row * SP;
    float m = -INFINITY;
    for (int t = lane; t < Tp; t += 64) m = fmaxf(m, sr[t]);
    m = wave_max_f32(m);
    float sum = 0.f;
    for (int t = lane; t < Tp; t += 64) {
      const float e = expf(sr[t] - m);
      sr[t] = e;
      sum += e;
    }
    sum = wave_sum_f32(sum);
    const bool keep = slot >= 0 && q0 + row < n;
    float* pr = keep ? a.probs + W.poff + ((int64_t)slot * n + q0 + row) * W.F : nullptr;
    for (int t = lane; t < Tp; t += 64) {
      const float p = sr[t] / sum;
      sr[t] = p;
      if (keep && t < W.F) pr[t] = p;
    }
  }
  __syncthreads();

  const int col = h * 64 + wid * 16 + l15;
  f32x4 o = zero_f32x4();
  for (int c = 0; c < Tp; c += 32) {
    const float* pp = sS + l15 * SP + c + 8 * lg;
    const float4 p0 = *reinterpret_cast<const float4*>(pp);
    const float4 p1 = *reinterpret_cast<const float4*>(pp + 4);
    const half8 pa = {(_Float16)p0.x, (_Float16)p0.y, (_Float16)p0.z, (_Float16)p0.w,
                      (_Float16)p1.x, (_Float16)p1.y, (_Float16)p1.z, (_Float16)p1.w};
    half8 vb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = min(c + 8 * lg + j, Tk - 1);
      vb[j] = a.v[(kbase + key) * a.ldkv + col];
    }
    o = mfma16(pa, vb, o);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = q0 + 4 * lg + r;
    if (row < n) a.out[((int64_t)W.row0 + row) * a.ldo + col] = (_Float16)o[r];
  }
}

void align_attention_launch(const AlignAttnArgs& a, int n_tiles, int H, int max_keys, hipStream_t s) {
  JANUS_CHECK(H >= 1 && H <= 32, "align attention: 1 .. 32 heads");
  JANUS_CHECK(a.ldq % 8 == 0 && a.ldkv % 8 == 0, "align attention: row strides must be multiples of 8");
  JANUS_CHECK(max_keys >= 1 && max_keys <= 2048, "align attention: 1 .. 2048 keys");
  if (n_tiles <= 0) return;
  const size_t lds = (size_t)kAlignTileRows * (((max_keys + 31) & ~31) + 4) * sizeof(float);
  allow_dynamic_lds<align_attn_kernel>(160 * 1024);
  align_attn_kernel<<<dim3(n_tiles, H), 256, lds, s>>>(a);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ reduce
// mean and population std over the window's n rows, per (head, frame): fp64, two passes
__global__ __launch_bounds__(256) void align_stats_kernel(const float* __restrict__ probs,
                                                          const AlignWinDev* __restrict__ wins,
                                                          int heads, double* __restrict__ stats) {
  const AlignWinDev W = wins[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)heads * W.F) return;
  const int hd = (int)(i / W.F), t = (int)(i % W.F);
  const float* p = probs + W.poff + (int64_t)hd * W.n * W.F + t;
  double s = 0.0;
  for (int r = 0; r < W.n; ++r) s += (double)p[(int64_t)r * W.F];
  const double mean = s / W.n;
  double q = 0.0;
  for (int r = 0; r < W.n; ++r) {
    const double e = (double)p[(int64_t)r * W.F] - mean;
    q += e * e;
  }
  stats[2 * (W.soff + i)] = mean;
  stats[2 * (W.soff + i) + 1] = sqrt(q / W.n);
}

__global__ __launch_bounds__(256) void align_reduce_kernel(const float* __restrict__ probs,
                                                           const AlignWinDev* __restrict__ wins,
                                                           int heads, int sot_len,
                                                           const double* __restrict__ stats,
                                                           float* __restrict__ A) {
  const AlignWinDev W = wins[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)W.N * W.F) return;
  const int r = (int)(i / W.F), t = (int)(i % W.F);
  const int F = W.F;
  const bool filt = F > kAlignMedian / 2;
  double acc = 0.0;
  for (int hd = 0; hd < heads; ++hd) {
    const float* p = probs + W.poff + ((int64_t)hd * W.n + sot_len + r) * F;
    const double* st = stats + 2 * (W.soff + (int64_t)hd * F);
    if (!filt) {
      acc += ((double)p[t] - st[2 * t]) / st[2 * t + 1];
      continue;
    }
    double z[kAlignMedian];
#pragma unroll
    for (int k = 0; k < kAlignMedian; ++k) {
      int u = t + k - kAlignMedian / 2;   // reflect padding: -k -> k, F - 1 + k -> F - 1 - k
      if (u < 0) u = -u;
      if (u >= F) u = 2 * (F - 1) - u;
      z[k] = ((double)p[u] - st[2 * u]) / st[2 * u + 1];
    }
#pragma unroll
    for (int k = 1; k < kAlignMedian; ++k) {   // insertion sort: the median is z[3]
#pragma unroll
      for (int j = k; j > 0; --j) {
        const double lo = z[j - 1], hi = z[j];
        const bool sw = hi < lo;
        z[j - 1] = sw ? hi : lo;
        z[j] = sw ? lo : hi;
      }
    }
    acc += z[kAlignMedian / 2];
  }
  A[W.aoff + i] = (float)(acc / heads);
}

void align_reduce_launch(const float* probs, const AlignWinDev* wins, int n_windows, int heads,
                         int sot_len, int max_n, int max_F, double* stats, float* A, hipStream_t s) {
  JANUS_CHECK(heads >= 1 && heads <= kAlignMaxHeads, "align reduce: 1 .. 64 heads");
  if (n_windows <= 0 || max_F <= 0 || max_n <= 0) return;
  align_stats_kernel<<<dim3((unsigned)cdiv((int64_t)heads * max_F, 256), n_windows), 256, 0, s>>>(
      probs, wins, heads, stats);
  JANUS_LAUNCH_CHECK();
  align_reduce_kernel<<<dim3((unsigned)cdiv((int64_t)max_n * max_F, 256), n_windows), 256, 0, s>>>(
      probs, wins, heads, sot_len, stats, A);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ DTW
// cost[i][j] = x[i-1][j-1] + min(cost[i-1][j-1], cost[i-1][j], cost[i][j-1]), border +inf but
// cost[0][0] = 0; trace = 0 if c0 < c1 && c0 < c2, else 1 if c1 < c0 && c1 < c2, else 2 (OpenAI's
// comparison order). Diagonal k = i + j: thread i owns row i of
// the cost matrix (N + 1 <= 512 rows), so it walks row i - 1 of x and row i of the trace
// left to right, one element per diagonal, and prefetches the next x before the barrier.
constexpr int kDtwThreads = 512;

__global__ __launch_bounds__(kDtwThreads) void align_dtw_kernel(
    const float* __restrict__ A, const AlignWinDev* __restrict__ wins, int negate,
    uint8_t* __restrict__ trace, int32_t* __restrict__ rev, int32_t* __restrict__ text_idx,
    int32_t* __restrict__ time_idx, int32_t* __restrict__ path_len, int path_stride) {
#pragma clang fp contract(off)
  __shared__ float diag[3][kDtwThreads];
  __shared__ int s_len;
  const int w = blockIdx.x, i = threadIdx.x;
  const AlignWinDev W = wins[w];
  const int N = W.N, F = W.F;
  const float* x = A + W.aoff;
  uint8_t* tr = trace + W.toff;
  const bool inner = i >= 1 && i <= N;
  const float* xrow = x + (int64_t)(inner ? i - 1 : 0) * F;
  uint8_t* trow = tr + (int64_t)i * (F + 1);
  float xn = 0.f;
  for (int k = 0; k <= N + F; ++k) {
    float* cur = diag[k % 3];
    const float* p1 = diag[(k + 2) % 3];
    const float* p2 = diag[(k + 1) % 3];
    const int j = k - i;
    const float xv = negate ? -xn : xn;
    const int jn = j + 1;   // the element this thread needs on the next diagonal
    if (inner && jn >= 1 && jn <= F) xn = xrow[jn - 1];
    if (i <= N && j >= 0 && j <= F) {
      float c;
      if (i == 0 || j == 0) {
        c = k == 0 ? 0.f : INFINITY;
      } else {
        const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
        const uint8_t t = (c0 < c1 && c0 < c2) ? 0 : ((c1 < c0 && c1 < c2) ? 1 : 2);
        c = xv + fminf(fminf(c0, c1), c2);
        trow[j] = t;
      }
      cur[i] = c;
    }
    __syncthreads();
  }
  int32_t* rt = rev + (int64_t)w * 2 * path_stride;
  int32_t* rf = rt + path_stride;
  if (i == 0) {
    int a = N, b = F, L = 0;
    while ((a > 0 || b > 0) && L < path_stride) {
      rt[L] = a - 1;
      rf[L] = b - 1;
      ++L;
      const int t = a == 0 ? 2 : (b == 0 ? 1 : tr[(int64_t)a * (F + 1) + b]);
      if (t == 0) { --a; --b; }
      else if (t == 1) --a;
      else --b;
    }
    s_len = L;
    path_len[w] = L;
  }
  __syncthreads();
  const int L = s_len;
  for (int k = i; k < path_stride; k += kDtwThreads) {
    text_idx[(int64_t)w * path_stride + k] = k < L ? rt[L - 1 - k] : -1;
    time_idx[(int64_t)w * path_stride + k] = k < L ? rf[L - 1 - k] : -1;
  }
}

void align_dtw_launch(const float* A, const AlignWinDev* wins, int n_windows, int negate,
                      uint8_t* trace, int32_t* rev, int32_t* text_idx, int32_t* time_idx,
                      int32_t* path_len, int path_stride, hipStream_t s) {
  if (n_windows <= 0) return;
  align_dtw_kernel<<<n_windows, kDtwThreads, 0, s>>>(A, wins, negate, trace, rev, text_idx, time_idx,
                                                     path_len, path_stride);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ forced-token probability
__global__ __launch_bounds__(256) void align_rowprob_kernel(const float* __restrict__ logits, int64_t ld,
                                                            int V, const int32_t* __restrict__ target,
                                                            const int32_t* __restrict__ out_idx,
                                                            float* __restrict__ out) {
  __shared__ float red[4];
  const int r = blockIdx.x, oi = out_idx[r];
  if (oi < 0) return;   // uniform over the block
  const float* l = logits + (int64_t)r * ld;
  const int lane = threadIdx.x & 63, wid = wave_id();
  float m = -INFINITY;
  for (int c = threadIdx.x; c < V; c += 256) m = fmaxf(m, l[c]);
  m = wave_max_f32(m);
  if (lane == 0) red[wid] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) sum += expf(l[c] - m);
  sum = wave_sum_f32(sum);
  if (lane == 0) red[wid] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    out[oi] = expf(l[min(max(target[r], 0), V - 1)] - m) / tot;
  }
}

void align_rowprob_launch(const float* logits, int64_t ld, int V, const int32_t* target,
                          const int32_t* out_idx, int rows, float* out, hipStream_t s) {
  if (rows <= 0 || V <= 0) return;
  align_rowprob_kernel<<<rows, 256, 0, s>>>(logits, ld, V, target, out_idx, out);
  JANUS_LAUNCH_CHECK();
}

}  // namespace janus

// Beam search (beam_size 2 .. 8) on top of the greedy decoder's launches.
//
// Rows are windows x k; the vocabulary projection's beam instantiation (decoder.hip) leaves
// per (row, block) the block's best 16 allowed entries beside the filtered statistics. Here:
//   beam_step_kernel     one block per window: the rows' statistics, the timestamp-mass
//                        rule per beam, the window's best 2k candidates by cumulative score,
//                        the walk (eot candidates finish, the others become the next live
//                        beams), the children's tokens / scores / rule states;
//   beam_reorder_kernel  the self-attention K / V caches follow the parents, in place;
//   beam_finish_kernel   the winner of every window into the call's outputs.
// The rule is stated in include/janus.h (janus_whisper_decode_beam_ex) and DESIGN.md §5k.
#include <cfloat>
#include "mfma.h"
#include "kernels.h"
#include "decoder.h"
#include "decoder_dev.h"

namespace janus {

__global__ void beam_init_kernel(BeamState st, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < W) { st.nlive[i] = 1; st.nfin[i] = 0; st.wdone[i] = 0; st.moved[i] = 0; }
  if (i < W * st.k) st.parent[i] = i % st.k;
}

void beam_init_launch(const BeamState& st, int W, hipStream_t s) {
  beam_init_kernel<<<(W * st.k + 63) / 64, 64, 0, s>>>(st, W);
  JANUS_LAUNCH_CHECK();
}

// (logit, index) as one integer that orders like `better`: larger logit first, then the
// smaller index; an empty slot is 0 (below every entry: an entry's low word is >= 2^31)
__device__ __forceinline__ unsigned long long beam_key(float v, int i) {
  if (i == 0x7fffffff) return 0ull;
  const uint32_t u = __float_as_uint(v);
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)ord << 32) | (uint32_t)(0xffffffffu - (uint32_t)i);
}
__device__ __forceinline__ float beam_key_val(unsigned long long k) {
  const uint32_t ord = (uint32_t)(k >> 32);
  return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord);
}
__device__ __forceinline__ int beam_key_idx(unsigned long long k) {
  return (int)(0xffffffffu - (uint32_t)(k & 0xffffffffu));
}

// One wave stages the first n entries of a row's nblk (<= 256) sorted lists (set 0: every
// allowed token, 1: the allowed timestamps) as keys, key[slot * nblk + list].
__device__ __forceinline__ void beam_stage_keys(const BeamTop* __restrict__ tp, int nblk, int set, int n,
                                                unsigned long long* key, int lane) {
  for (int e = lane; e < nblk * n; e += 64) {
    const int q = e / nblk, l = e - q * nblk;
    key[e] = set ? beam_key(tp[l].tv[q], tp[l].ti[q]) : beam_key(tp[l].av[q], tp[l].ai[q]);
  }
}

// One wave, after the staging is visible: the best n entries over the lists, in order, to
// ov / oi (lane 0 writes); returns how many exist. Lane l owns lists l, l + 64, l + 128,
// l + 192 and a cursor into each; every round takes the wave's largest head.
__device__ __forceinline__ int beam_select_keys(const unsigned long long* key, int nblk, int n,
                                                float* ov, int* oi, int lane) {
  int hp[4] = {0, 0, 0, 0};
  int cnt = 0;
  for (int r = 0; r < n; ++r) {
    unsigned long long best = 0ull;
    int bq = 0;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int l = lane + 64 * q4;
      const unsigned long long h = (l < nblk && hp[q4] < n) ? key[hp[q4] * nblk + l] : 0ull;
      if (h > best) { best = h; bq = q4; }
    }
    unsigned long long wb = best;
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(wb, o);
      wb = other > wb ? other : wb;
    }
    if (wb == 0ull) break;  // wave-uniform: the lists are exhausted
    if (best == wb) {       // keys are unique (a token lies in one block): one owner
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4)
        if (q4 == bq) hp[q4] += 1;
    }
    if (lane == 0) { ov[r] = beam_key_val(wb); oi[r] = beam_key_idx(wb); }
    cnt = r + 1;
  }
  return cnt;
}

constexpr int kBeamTokMax = 448;  // n_text_ctx of every Whisper model

__global__ __launch_bounds__(256) void beam_step_kernel(
    const LogitPart* __restrict__ parts, const BeamTop* __restrict__ tops, int nblk, DecodeRules R,
    RowRules* __restrict__ rules, int32_t* __restrict__ tokens, int ld, int pos,
    int32_t* __restrict__ done, float* __restrict__ sum_lp, int32_t* __restrict__ n_tok,
    const int32_t* __restrict__ plen, float* __restrict__ nsp, BeamState st) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long bm_keys[];  // [4 waves][n2k][nblk]
  __shared__ LogitPart sh[4];
  __shared__ float s_lse[kBeamMax], s_S[kBeamMax];
  __shared__ int s_set[kBeamMax], s_cnt[kBeamMax], s_ntok[kBeamMax];
  __shared__ RowRules s_rules[kBeamMax];
  __shared__ float s_cv[kBeamMax][kBeamTop];
  __shared__ int s_ci[kBeamMax][kBeamTop];
  __shared__ int s_par[kBeamMax], s_tok[kBeamMax], s_fpar[kBeamMax];
  __shared__ float s_nS[kBeamMax], s_fS[kBeamMax];
  __shared__ int s_nnew, s_nfin0, s_nfin1;
  __shared__ int32_t s_hist[kBeamMax * kBeamTokMax];
  const int wdw = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int k = st.k, n2k = 2 * k, b0 = wdw * k;
  const int pl = plen[b0];  // the window's rows share its prompt
  if (pos + 1 < pl) {       // inside the prompt: the forced tokens stay, parents the identity
    // no_speech_prob read before the prompt's end (janus_decode_rows.no_speech_back), as
    // select_row: beam 0's raw statistics, nothing else touched (block-uniform)
    if (nsp && pos + 1 + R.target_back == pl) {
      const LogitPart q = row_parts_reduce(parts + (int64_t)b0 * nblk, nblk, sh);
      if (tid == 0) nsp[b0] = R.target >= 0 ? __expf(q.t_v - (q.m_raw + __logf(q.s_raw))) : 0.f;
    }
    if (tid == 0) st.moved[wdw] = 0;
    return;
  }
  if (st.wdone[wdw]) {      // a stopped window idles on eot
    if (tid < k) tokens[(int64_t)(b0 + tid) * ld + pos + 1] = R.eot;
    if (tid == 0) st.moved[wdw] = 0;
    return;
  }
  const int nlive = st.nlive[wdw];
  // the live rows' token histories (positions 0 .. pos) and states
  for (int e = tid; e < nlive * (pos + 1); e += 256) {
    const int j = e / (pos + 1), p = e - j * (pos + 1);
    s_hist[j * kBeamTokMax + p] = tokens[(int64_t)(b0 + j) * ld + p];
  }
  if (tid < nlive) {
    s_S[tid] = sum_lp[b0 + tid];
    s_ntok[tid] = n_tok[b0 + tid];
    s_rules[tid] = rules[b0 + tid];
  }
  // per live beam: the filtered statistics and the timestamp-mass rule, as select_row
  for (int j = 0; j < nlive; ++j) {
    __syncthreads();  // sh free again
    const LogitPart q = row_parts_reduce(parts + (int64_t)(b0 + j) * nblk, nblk, sh);
    if (tid == 0) {
      if (j == 0 && nsp && pos + 1 + R.target_back == pl)
        nsp[b0] = R.target >= 0 ? __expf(q.t_v - (q.m_raw + __logf(q.s_raw))) : 0.f;
      const float lse_all = q.m_all + __logf(q.s_all);
      float lse = lse_all;
      int set = 0;
      if (R.ts_begin >= 0 && q.m_ts > -INFINITY) {
        const float lse_ts = q.m_ts + __logf(q.s_ts);
        if (lse_ts - lse_all > q.m_text - lse_all) { set = 1; lse = lse_ts; }
      }
      s_lse[j] = lse;
      s_set[j] = set;
    }
  }
  __syncthreads();
  // per live beam: its best 2k entries of the applicable set (one wave per beam, two rounds)
  unsigned long long* key = bm_keys + (size_t)w * n2k * nblk;
  for (int j0 = 0; j0 < nlive; j0 += 4) {
    const int j = j0 + w;
    if (j < nlive) beam_stage_keys(tops + (int64_t)(b0 + j) * nblk, nblk, s_set[j], n2k, key, lane);
    __syncthreads();
    if (j < nlive) {
      const int c = beam_select_keys(key, nblk, n2k, s_cv[j], s_ci[j], lane);
      if (lane == 0) s_cnt[j] = c;
    }
    __syncthreads();
  }
  // the window's best 2k candidates by S + log-prob (then beam, then token), walked
  if (tid == 0) {
    int hp[kBeamMax];
    for (int j = 0; j < nlive; ++j) hp[j] = 0;
    int nnew = 0, nfin = st.nfin[wdw];
    s_nfin0 = nfin;
    for (int r = 0; r < n2k && nnew < k; ++r) {
      int bj = -1, bv = 0;
      float bs = 0.f;
      for (int j = 0; j < nlive; ++j) {
        if (hp[j] >= s_cnt[j]) continue;
        const float sc = s_S[j] + (s_cv[j][hp[j]] - s_lse[j]);
        const int v = s_ci[j][hp[j]];
        // rows are visited in beam order: a later beam wins on a strictly larger score only
        if (bj < 0 || sc > bs) { bj = j; bs = sc; bv = v; }
      }
      if (bj < 0) break;
      hp[bj] += 1;
      if (bv == R.eot) {
        if (nfin < k) { s_fpar[nfin] = bj; s_fS[nfin] = bs; nfin += 1; }
      } else {
        s_par[nnew] = bj; s_tok[nnew] = bv; s_nS[nnew] = bs; nnew += 1;
      }
    }
    s_nnew = nnew;
    s_nfin1 = nfin;
  }
  __syncthreads();
  const int nnew = s_nnew, nfin0 = s_nfin0, nfin1 = s_nfin1;
  // children: the parent's history, then the new token; the other rows idle on eot
  for (int e = tid; e < nnew * (pos + 1); e += 256) {
    const int i = e / (pos + 1), p = e - i * (pos + 1);
    if (s_par[i] != i) tokens[(int64_t)(b0 + i) * ld + p] = s_hist[s_par[i] * kBeamTokMax + p];
  }
  // finished this step: prompt, the parent's sampled tokens, eot
  for (int e = tid; e < (nfin1 - nfin0) * (pos + 2); e += 256) {
    const int f = nfin0 + e / (pos + 2), p = e % (pos + 2);
    st.fin_tok[((int64_t)wdw * k + f) * ld + p] = p <= pos ? s_hist[s_fpar[f] * kBeamTokMax + p] : R.eot;
  }
  const bool stop = nfin1 >= k || nnew == 0;
  if (tid < k) {
    const int i = tid, b = b0 + i;
    if (i < nnew) {
      const int pj = s_par[i];
      tokens[(int64_t)b * ld + pos + 1] = s_tok[i];
      sum_lp[b] = s_nS[i];
      n_tok[b] = s_ntok[pj] + 1;
      rules[b] = next_row_rules(s_rules[pj], R, s_hist[pj * kBeamTokMax + pos], s_tok[i]);
      st.parent[b] = pj;
    } else {
      tokens[(int64_t)b * ld + pos + 1] = R.eot;
      st.parent[b] = i;
    }
    if (stop) done[b] = 1;
    if (i >= nfin0 && i < nfin1) {
      st.fin_s[wdw * k + i] = s_fS[i];
      st.fin_n[wdw * k + i] = s_ntok[s_fpar[i]] + 1;
    }
  }
  if (tid == 0) {
    int mv = 0;
    for (int i = 0; i < nnew; ++i) mv |= (s_par[i] != i);
    st.moved[wdw] = mv;
    st.nfin[wdw] = nfin1;
    // a stopped window keeps its live beams as they stood (the winner comes from the
    // finished list; with no candidate left at all there is nothing to continue)
    if (stop) st.wdone[wdw] = 1;
    else st.nlive[wdw] = nnew;
  }
}

void beam_step_launch(const SelectArgs& a, const BeamTop* tops, const BeamState& st, int W, hipStream_t s) {
  JANUS_CHECK(st.k >= 1 && st.k <= kBeamMax, "beam_step: beam size must be 1 .. 8");
  JANUS_CHECK(a.nblk >= 1 && a.nblk <= 256, "beam_step: 1 .. 256 partials per row");
  JANUS_CHECK(a.ld <= kBeamTokMax && a.pos + 1 < a.ld, "beam_step: max_length <= 448, pos + 1 < max_length");
  JANUS_CHECK(a.plen, "beam_step: per-row prompt lengths needed");
  const size_t lds = (size_t)4 * 2 * st.k * a.nblk * sizeof(unsigned long long);
  allow_dynamic_lds<beam_step_kernel>(4 * kBeamTop * 256 * (int)sizeof(unsigned long long));
  beam_step_kernel<<<W, 256, lds, s>>>(a.parts, tops, a.nblk, a.R, a.rules, a.tokens, a.ld, a.pos, a.done,
                                       a.sum_lp, a.n_tok, a.plen, a.nsp, st);
  JANUS_LAUNCH_CHECK();
}

// --------------------------------------------------------------------- KV reorder
// Block (chunk c, layer * 2 + K-or-V, window): positions [8 c, 8 c + 8) up to pos of every
// row of the window. A thread owns the same uint4 elements of all k rows: it loads the rows
// some child needs, then stores each moved row from its parent's registers — parents are a
// map, not a permutation, and nothing is read after the first store.
constexpr int kReorderPos = 8;   // positions per block
constexpr int kReorderU = 3;     // uint4 per thread and row: 8 positions x d / 8 <= 768 at d = 768

__global__ __launch_bounds__(256) void beam_reorder_kernel(_Float16* __restrict__ kc, _Float16* __restrict__ vc,
                                                           int B, int k, int n_ctx, int d, int pos,
                                                           const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ moved) {
  const int wdw = blockIdx.z;
  if (!moved[wdw]) return;  // block-uniform: identity parents
  const int layer = blockIdx.y >> 1;
  _Float16* base = (blockIdx.y & 1) ? vc : kc;
  const int p0 = blockIdx.x * kReorderPos;
  const int np = min(kReorderPos, pos + 1 - p0);       // positions of this chunk (>= 1 by the grid)
  const int ne = np * (d / 8);                         // uint4 elements per row
  int par[kBeamMax];
  unsigned need = 0;                                   // rows some other row takes
#pragma unroll
  for (int i = 0; i < kBeamMax; ++i) {
    par[i] = i < k ? parent[wdw * k + i] : i;
    if (par[i] != i) need |= 1u << par[i];
  }
  const int64_t row_stride = (int64_t)n_ctx * d;       // halves between rows
  uint4* rows0 = reinterpret_cast<uint4*>(base + ((int64_t)layer * B + (int64_t)wdw * k) * row_stride +
                                          (int64_t)p0 * d);
  const int64_t rs4 = row_stride / 8;
  uint4 r[kBeamMax][kReorderU];
#pragma unroll
  for (int j = 0; j < kBeamMax; ++j)
#pragma unroll
    for (int u = 0; u < kReorderU; ++u) {
      const int e = threadIdx.x + 256 * u;
      r[j][u] = make_uint4(0, 0, 0, 0);
      if (j < k && ((need >> j) & 1u) && e < ne) r[j][u] = rows0[j * rs4 + e];
    }
  // (each thread reads and writes its own elements only: no exchange between threads)
#pragma unroll
  for (int i = 0; i < kBeamMax; ++i) {
    if (i >= k || par[i] == i) continue;
#pragma unroll
    for (int u = 0; u < kReorderU; ++u) {
      const int e = threadIdx.x + 256 * u;
      uint4 v = r[0][u];
#pragma unroll
      for (int j = 1; j < kBeamMax; ++j)
        if (par[i] == j) v = r[j][u];
      if (e < ne) rows0[i * rs4 + e] = v;
    }
  }
}

void beam_reorder_launch(_Float16* kc, _Float16* vc, int layers, int W, int k, int n_ctx, int d,
                         int pos, const int32_t* parent, const int32_t* moved, hipStream_t s) {
  JANUS_CHECK(k >= 1 && k <= kBeamMax, "beam_reorder: beam size must be 1 .. 8");
  JANUS_CHECK(d % 8 == 0 && kReorderPos * (d / 8) <= 256 * kReorderU, "beam_reorder: d <= 768, a multiple of 8");
  JANUS_CHECK(pos >= 0 && pos < n_ctx, "beam_reorder: pos out of range");
  JANUS_CHECK(W >= 1 && W <= 65535 && layers >= 1, "beam_reorder: bad shape");
  if (k == 1) return;  // one beam: its own parent
  const dim3 grid((unsigned)cdiv(pos + 1, kReorderPos), (unsigned)(2 * layers), (unsigned)W);
  beam_reorder_kernel<<<grid, 256, 0, s>>>(kc, vc, W * k, k, n_ctx, d, pos, parent, moved);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------- finish
__global__ __launch_bounds__(256) void beam_finish_kernel(
    BeamState st, DecodeRules R, const int32_t* __restrict__ tokens, int ld,
    const float* __restrict__ sum_lp, const int32_t* __restrict__ n_tok,
    const int32_t* __restrict__ plen, const float* __restrict__ nsp, int32_t* __restrict__ tokens_out,
    int32_t* __restrict__ n_tokens_out, float* __restrict__ sum_lp_out, float* __restrict__ nsp_out) {
  __shared__ int s_src, s_n;  // winner: finished slot f -> f, live beam i -> k + i
  const int wdw = blockIdx.x, k = st.k, b0 = wdw * k;
  if (threadIdx.x == 0) {
    const float pen = st.length_penalty;
    auto norm = [&](float S, int n) { return pen == 1.0f ? S / (float)n : S / powf((float)n, pen); };
    const int nfin = st.nfin[wdw];
    int src = -1, n = 0;
    float best = 0.f, S = 0.f;
    for (int f = 0; f < nfin; ++f) {
      const float sc = norm(st.fin_s[b0 + f], st.fin_n[b0 + f]);
      if (src < 0 || sc > best) { src = f; best = sc; S = st.fin_s[b0 + f]; n = st.fin_n[b0 + f]; }
    }
    if (src < 0) {  // none finished: the live beams closed as they stand
      const int nlive = st.nlive[wdw];
      for (int i = 0; i < nlive; ++i) {
        const float sc = norm(sum_lp[b0 + i], n_tok[b0 + i] + 1);
        if (src < 0 || sc > best) { src = k + i; best = sc; S = sum_lp[b0 + i]; n = n_tok[b0 + i]; }
      }
    }
    if (src < 0) src = k;  // (no beam at all: row 0's prompt, nothing sampled)
    s_src = src; s_n = n;
    n_tokens_out[wdw] = n;
    sum_lp_out[wdw] = S;
    if (nsp_out) nsp_out[wdw] = nsp[b0];
  }
  __syncthreads();
  const int src = s_src, end = plen[b0] + s_n;
  const int32_t* row = src < k ? st.fin_tok + ((int64_t)b0 + src) * ld : tokens + ((int64_t)b0 + src - k) * ld;
  for (int p = threadIdx.x; p < ld; p += 256) tokens_out[(int64_t)wdw * ld + p] = p < end ? row[p] : -1;
}

void beam_finish_launch(const BeamState& st, const DecodeRules& R, const int32_t* tokens, int ld,
                        const float* sum_lp, const int32_t* n_tok, const int32_t* plen,
                        const float* nsp, int W, int32_t* tokens_out, int32_t* n_tokens_out,
                        float* sum_lp_out, float* nsp_out, hipStream_t s) {
  beam_finish_kernel<<<W, 256, 0, s>>>(st, R, tokens, ld, sum_lp, n_tok, plen, nsp, tokens_out,
                                       n_tokens_out, sum_lp_out, nsp_out);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------- kernel test
__global__ __launch_bounds__(64) void beam_rowtop_kernel(const BeamTop* __restrict__ tops, int nblk, int n2k,
                                                         float* __restrict__ all_v, int32_t* __restrict__ all_i,
                                                         float* __restrict__ ts_v, int32_t* __restrict__ ts_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rt_keys[];
  __shared__ float ov[kBeamTop];
  __shared__ int oi[kBeamTop];
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int set = 0; set < 2; ++set) {
    __syncthreads();
    beam_stage_keys(tops + (int64_t)b * nblk, nblk, set, n2k, rt_keys, lane);
    __syncthreads();
    const int c = beam_select_keys(rt_keys, nblk, n2k, ov, oi, lane);
    __syncthreads();
    if (lane < n2k) {
      (set ? ts_v : all_v)[(int64_t)b * n2k + lane] = lane < c ? ov[lane] : -INFINITY;
      (set ? ts_i : all_i)[(int64_t)b * n2k + lane] = lane < c ? oi[lane] : -1;
    }
  }
}

void beam_rowtop_launch(const BeamTop* tops, int nblk, int B, int n2k, float* all_v, int32_t* all_i,
                        float* ts_v, int32_t* ts_i, hipStream_t s) {
  JANUS_CHECK(n2k >= 1 && n2k <= kBeamTop && nblk >= 1 && nblk <= 256, "beam_rowtop: 2k <= 16, <= 256 partials");
  const size_t lds = (size_t)n2k * nblk * sizeof(unsigned long long);
  beam_rowtop_kernel<<<B, 64, lds, s>>>(tops, nblk, n2k, all_v, all_i, ts_v, ts_i);
  JANUS_LAUNCH_CHECK();
}

}  // namespace janus

#include <algorithm>
// Small kernels of the greedy Whisper decoder loop (batched over utterances, one
// token per step) and of the encoder/decoder glue.
//
// The token selector restates the logit filters faster-whisper's greedy path applies
// (transcribe(beam_size=1, language='en'), transcriber.py:53-57; CTranslate2
// Whisper generate with the OpenAI decoding rules: SuppressBlank, SuppressTokens,
// ApplyTimestampRules incl. max_initial_timestamp, then argmax) and accumulates the
// chosen token's log-probability (avg_logprob).
#include <cfloat>
#include <cstdlib>
#include <utility>
#ifdef JANUS_DEBUG_ASSERT
#include <cassert>
#endif
#include "mfma.h"
#include "kernels.h"
#include "decoder.h"
#include "decoder_dev.h"

namespace janus {

__global__ void cast_f16_f32_kernel(const _Float16* __restrict__ in, float* __restrict__ out,
                                    int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

void cast_f16_f32_launch(const _Float16* in, float* out, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  cast_f16_f32_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(in, out, n);
  JANUS_LAUNCH_CHECK();
}

__global__ void cast_f32_f16_kernel(const float* __restrict__ in, _Float16* __restrict__ out,
                                    int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (_Float16)in[i];
}

void cast_f32_f16_launch(const float* in, _Float16* out, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  cast_f32_f16_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(in, out, n);
  JANUS_LAUNCH_CHECK();
}

// x[b][:] = tok_emb[tokens[b][pos]] + pos_emb[pos]   (fp32 residual stream)
// 16-column LayerNorm piece (sum, M2 about the piece mean) of 16 values spread two per
// lane over 8 aligned lanes; every lane of the group returns it.
__device__ __forceinline__ float2 ln_piece8x2(float v0, float v1) {
  float s = v0 + v1;
  s += xshfl<1>(s);
  s += xshfl<2>(s);
  s += xshfl<4>(s);
  const float m = s * (1.0f / 16.0f);
  float q = (v0 - m) * (v0 - m) + (v1 - m) * (v1 - m);
  q += xshfl<1>(q);
  q += xshfl<2>(q);
  q += xshfl<4>(q);
  return make_float2(s, q);
}

// row b's embedding at position pos (token tok) -> x[b] (+ LayerNorm pieces / the first
// layer's LayerNorm of the row); 256 threads
__device__ __forceinline__ void embed_row(const _Float16* __restrict__ tok_emb,
                                          const float* __restrict__ pos_emb, int tok, int b,
                                          int pos, int d, float* __restrict__ x,
                                          float2* __restrict__ part, const float* __restrict__ ln_g,
                                          const float* __restrict__ ln_b,
                                          _Float16* __restrict__ ln_out) {
  __shared__ float red[2][4];
  // every token read here was written by a selection or the prompt: the context rejects a
  // staggered row continued past where its slot stands (janus_whisper_decode_stand), so
  // the -1 fill is never embedded (JANUS_DEBUG_ASSERT builds check it). Release builds
  // still clamp: a path that missed the host check embeds token 0 (wrong text, no fault)
  // instead of reading before tok_emb
#ifdef JANUS_DEBUG_ASSERT
  assert(tok >= 0);
#endif
  tok = max(tok, 0);
  float v0 = 0.f, v1 = 0.f;
  for (int base = 0; base < d; base += 512) {
    const int col = base + 2 * threadIdx.x;   // 8 lanes = one 16-column piece
    v0 = 0.f; v1 = 0.f;
    if (col < d) {
      v0 = (float)tok_emb[(int64_t)tok * d + col] + pos_emb[(int64_t)pos * d + col];
      v1 = (float)tok_emb[(int64_t)tok * d + col + 1] + pos_emb[(int64_t)pos * d + col + 1];
      *reinterpret_cast<float2*>(x + (int64_t)b * d + col) = make_float2(v0, v1);
    }
    if (part) {
      const float2 pc = ln_piece8x2(v0, v1);
      if (col < d && (threadIdx.x & 7) == 0) part[(int64_t)b * (d / 16) + col / 16] = pc;
    }
  }
  if (ln_out) {  // the first layer's LayerNorm of this row (d <= 512: one pass above)
    const int col = 2 * threadIdx.x, wv = threadIdx.x >> 6;
    const bool ok = col < d;
    float s = v0 + v1;
    s = wave_sum_f32(s);
    if ((threadIdx.x & 63) == 0) red[0][wv] = s;
    __syncthreads();
    const float mean = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / d;
    float q = ok ? (v0 - mean) * (v0 - mean) + (v1 - mean) * (v1 - mean) : 0.f;
    q = wave_sum_f32(q);
    if ((threadIdx.x & 63) == 0) red[1][wv] = q;
    __syncthreads();
    const float rstd = rsqrtf((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / d + 1e-5f);
    if (ok) {
      ln_out[(int64_t)b * d + col] = (_Float16)((v0 - mean) * rstd * ln_g[col] + ln_b[col]);
      ln_out[(int64_t)b * d + col + 1] = (_Float16)((v1 - mean) * rstd * ln_g[col + 1] + ln_b[col + 1]);
    }
  }
}

__global__ __launch_bounds__(256) void embed_kernel(const _Float16* __restrict__ tok_emb,
                                                    const float* __restrict__ pos_emb,
                                                    const int32_t* __restrict__ tokens,
                                                    int ld_tokens, int pos, int d,
                                                    float* __restrict__ x,
                                                    float2* __restrict__ part,
                                                    const float* __restrict__ ln_g,
                                                    const float* __restrict__ ln_b,
                                                    _Float16* __restrict__ ln_out,
                                                    const int32_t* __restrict__ roff) {
  const int b = blockIdx.x;
  const int pb = pos + (roff ? roff[b] : 0);  // the row's own position (staggered rows)
  embed_row(tok_emb, pos_emb, tokens[(int64_t)b * ld_tokens + pb], b, pb, d, x, part, ln_g, ln_b,
            ln_out);
}

void embed_launch(const _Float16* tok_emb, const float* pos_emb, const int32_t* tokens,
                  int ld_tokens, int pos, int d, float* x, float2* part, int B, hipStream_t s,
                  const float* ln_g, const float* ln_b, _Float16* ln_out, const int32_t* roff) {
  JANUS_CHECK(d % 16 == 0, "embed: d % 16 != 0");
  JANUS_CHECK(!ln_out || d <= 512, "embed: fused LayerNorm needs d <= 512");
  embed_kernel<<<B, 256, 0, s>>>(tok_emb, pos_emb, tokens, ld_tokens, pos, d, x, part, ln_g, ln_b,
                                 ln_out, roff);
  JANUS_LAUNCH_CHECK();
}

// qkv[b][d:3d] -> kcache[b][pos][:], vcache[b][pos][:]
__global__ void kv_store_kernel(const _Float16* __restrict__ qkv, int d, int pos, int n_ctx,
                                _Float16* __restrict__ kc, _Float16* __restrict__ vc) {
  const int b = blockIdx.x;
  const _Float16* src = qkv + (int64_t)b * 3 * d;
  _Float16* kd = kc + ((int64_t)b * n_ctx + pos) * d;
  _Float16* vd = vc + ((int64_t)b * n_ctx + pos) * d;
  for (int i = threadIdx.x; i < d; i += blockDim.x) {
    kd[i] = src[d + i];
    vd[i] = src[2 * d + i];
  }
}

void kv_store_launch(const _Float16* qkv, int d, int pos, int n_ctx, _Float16* kc, _Float16* vc,
                     int B, hipStream_t s) {
  kv_store_kernel<<<B, 256, 0, s>>>(qkv, d, pos, n_ctx, kc, vc);
  JANUS_LAUNCH_CHECK();
}

__global__ void init_tokens_kernel(int32_t* tokens, int ld, const int32_t* prompt, int plen,
                                   int32_t* done, float* sum_lp, int32_t* n_tok) {
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < ld; i += blockDim.x)
    tokens[(int64_t)b * ld + i] = i < plen ? prompt[i] : -1;
  if (threadIdx.x == 0) { done[b] = 0; sum_lp[b] = 0.f; n_tok[b] = 0; }
}

void init_tokens_launch(int32_t* tokens, int ld, const int32_t* prompt, int plen, int32_t* done,
                        float* sum_lp, int32_t* n_tok, int B, hipStream_t s) {
  init_tokens_kernel<<<B, 256, 0, s>>>(tokens, ld, prompt, plen, done, sum_lp, n_tok);
  JANUS_LAUNCH_CHECK();
}

__global__ void init_counters_kernel(int32_t* done, float* sum_lp, int32_t* n_tok, float* nsp, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  done[b] = 0;
  sum_lp[b] = 0.f;
  n_tok[b] = 0;
  if (nsp) nsp[b] = 0.f;
}

void init_counters_launch(int32_t* done, float* sum_lp, int32_t* n_tok, float* nsp, int B,
                          hipStream_t s) {
  init_counters_kernel<<<(B + 63) / 64, 64, 0, s>>>(done, sum_lp, n_tok, nsp, B);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ select
// the rules past the suppress mask, for a token whose mask byte is already in a register
__device__ __forceinline__ bool allowed_unmasked(int t, const DecodeRules& R, const RowRules& rr,
                                                 bool ban_all_text);

__device__ __forceinline__ bool allowed(int t, const uint8_t* smask, const DecodeRules& R,
                                        const RowRules& rr, bool ban_all_text) {
  if (smask[t]) return false;
  return allowed_unmasked(t, R, rr, ban_all_text);
}

__device__ __forceinline__ bool allowed_unmasked(int t, const DecodeRules& R, const RowRules& rr,
                                                 bool ban_all_text) {
  if (rr.sample_begin && R.suppress_blank && (t == R.blank || t == R.eot)) return false;
  if (R.ts_begin >= 0) {
    if (t == R.no_timestamps) return false;
    const bool is_ts = t >= R.ts_begin;
    if (rr.suppress_all_ts && is_ts) return false;
    if (rr.suppress_text && t < R.eot) return false;
    if (is_ts && t < rr.ts_floor) return false;
    if (rr.sample_begin) {
      if (!is_ts) return false;
      if (R.max_initial_ts >= 0 && t > R.ts_begin + R.max_initial_ts) return false;
    }
    if (ban_all_text && !is_ts) return false;
  }
  return true;
}

template <class Op>
__device__ __forceinline__ float block_reduce(float v, float* red, Op op) {
  v = op(v, xshfl<32>(v)); v = op(v, xshfl<16>(v)); v = op(v, xshfl<8>(v));
  v = op(v, xshfl<4>(v)); v = op(v, xshfl<2>(v)); v = op(v, xshfl<1>(v));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = op(r, red[k]);
  return r;
}

__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ logits, int V,
                                                     DecodeRules R, const uint8_t* __restrict__ smask,
                                                     int32_t* __restrict__ tokens, int ld, int pos,
                                                     int sample_begin_pos, int32_t* __restrict__ done,
                                                     float* __restrict__ sum_lp,
                                                     int32_t* __restrict__ n_tok) {
  __shared__ float red[8];
  __shared__ RowRules rr;
  __shared__ unsigned long long best;
  const int b = blockIdx.x, tid = threadIdx.x;
  int32_t* row_tok = tokens + (int64_t)b * ld;
  if (done[b]) {
    if (tid == 0) row_tok[pos + 1] = R.eot;
    return;
  }
  __shared__ int last_ts_pos;
  const int nsamp = pos + 1 - sample_begin_pos;  // tokens sampled so far
  if (tid == 0) { last_ts_pos = -1; best = 0ull; }
  __syncthreads();
  if (R.ts_begin >= 0) {
    int lp = -1;
    for (int i = sample_begin_pos + tid; i <= pos; i += blockDim.x)
      if (row_tok[i] >= R.ts_begin) lp = i;
    if (lp >= 0) atomicMax(&last_ts_pos, lp);
  }
  __syncthreads();
  if (tid == 0) {
    rr.sample_begin = nsamp == 0;
    rr.suppress_all_ts = rr.suppress_text = 0;
    rr.ts_floor = -1;
    rr.last_stamp = -1;
    if (R.ts_begin >= 0 && nsamp > 0) {
      const bool last_ts = row_tok[pos] >= R.ts_begin;
      const bool pen_ts = nsamp < 2 || row_tok[pos - 1] >= R.ts_begin;
      if (last_ts) {
        if (pen_ts) rr.suppress_all_ts = 1;
        else rr.suppress_text = 1;
      }
      if (last_ts_pos >= 0) {
        const int last_stamp = row_tok[last_ts_pos];
        rr.ts_floor = (last_ts && !pen_ts) ? last_stamp : last_stamp + 1;
      }
    }
  }
  __syncthreads();
  const RowRules rl = rr;
  const float* L = logits + (int64_t)b * V;

  // pass 1: maxima (all allowed, text, timestamps)
  float m_all = -INFINITY, m_text = -INFINITY, m_ts = -INFINITY;
  for (int t = tid; t < V; t += 256) {
    if (!allowed(t, smask, R, rl, false)) continue;
    const float v = L[t];
    m_all = fmaxf(m_all, v);
    if (R.ts_begin >= 0 && t >= R.ts_begin) m_ts = fmaxf(m_ts, v);
    else m_text = fmaxf(m_text, v);
  }
  auto fmax_op = [](float a, float c) { return fmaxf(a, c); };
  auto add_op = [](float a, float c) { return a + c; };
  m_all = block_reduce(m_all, red, fmax_op);
  m_text = block_reduce(m_text, red, fmax_op);
  m_ts = block_reduce(m_ts, red, fmax_op);
  // pass 2: partition sums
  float s_all = 0.f, s_ts = 0.f;
  for (int t = tid; t < V; t += 256) {
    if (!allowed(t, smask, R, rl, false)) continue;
    const float v = L[t];
    s_all += __expf(v - m_all);
    if (R.ts_begin >= 0 && t >= R.ts_begin) s_ts += __expf(v - m_ts);
  }
  s_all = block_reduce(s_all, red, add_op);
  s_ts = block_reduce(s_ts, red, add_op);
  const float lse_all = m_all + __logf(s_all);
  bool ban_text = false;
  float lse_final = lse_all;
  if (R.ts_begin >= 0 && m_ts > -INFINITY) {
    const float ts_lp = m_ts + __logf(s_ts) - lse_all;   // logsumexp of timestamp logprobs
    const float text_lp = m_text - lse_all;              // max text-token logprob
    if (ts_lp > text_lp) {
      ban_text = true;
      lse_final = m_ts + __logf(s_ts);
    }
  }
  // pass 3: argmax (first index on ties)
  unsigned long long key = 0ull;
  for (int t = tid; t < V; t += 256) {
    if (!allowed(t, smask, R, rl, ban_text)) continue;
    const uint32_t u = __float_as_uint(L[t]);
    const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const unsigned long long k = ((unsigned long long)ord << 32) | (uint32_t)(0xffffffffu - t);
    key = k > key ? k : key;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0) atomicMax(&best, key);
  __syncthreads();
  if (tid == 0) {
    const int next = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    row_tok[pos + 1] = next;
    sum_lp[b] += L[next] - lse_final;
    n_tok[b] += 1;
    if (next == R.eot) done[b] = 1;
  }
}

void select_launch(const float* logits, int V, const DecodeRules& R, const uint8_t* smask,
                   int32_t* tokens, int ld, int pos, int sample_begin_pos, int32_t* done,
                   float* sum_lp, int32_t* n_tok, int B, hipStream_t s) {
  select_kernel<<<B, 256, 0, s>>>(logits, V, R, smask, tokens, ld, pos, sample_begin_pos, done,
                                  sum_lp, n_tok);
  JANUS_LAUNCH_CHECK();
}

__global__ void build_mask_kernel(const int32_t* __restrict__ list, int n, uint8_t* __restrict__ mask,
                                  int V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && list[i] >= 0 && list[i] < V) mask[list[i]] = 1;
}


// ------------------------------------------------------- fused logits path
__global__ void rules_init_kernel(RowRules* rules, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  RowRules r;
  r.sample_begin = 1;
  r.suppress_all_ts = r.suppress_text = 0;
  r.ts_floor = -1;
  r.last_stamp = -1;
  r.pad[0] = r.pad[1] = r.pad[2] = 0;
  rules[b] = r;
}

void rules_init_launch(RowRules* rules, int B, hipStream_t s) {
  rules_init_kernel<<<(B + 63) / 64, 64, 0, s>>>(rules, B);
  JANUS_LAUNCH_CHECK();
}

// one merged partial per (row, block): the grid of logits_partial_kernel
// waves per logits block (16 waves — about one tile per wave — measured 4x slower:
// 114.7 vs 28.8 us per launch)
constexpr int lg_waves(int /*K*/) { return 8; }
// The widths the projection is built for: K = d_model and MT, the 16-row m-tiles of A per row
// group (why 3 at K = 1024 and 2 at K = 1280: at logits_partial_kernel below). The k-steps,
// the row group, the LDS size and the kernel table all derive from a row of this list.
struct LgWidth {
  int K, MT;
  constexpr int nks() const { return K / 32; }
  constexpr int rows() const { return 16 * MT; }
  // A [rows][K + 16] fp16, the waves' patches [waves][rows][17] f32, the rows' rules
  constexpr size_t lds() const {
    return (size_t)rows() * (K + 16) * 2 + (size_t)lg_waves(K) * rows() * 17 * 4 + 64 * sizeof(RowRules);
  }
};
constexpr LgWidth kLgWidths[] = {{384, 4}, {512, 4}, {768, 4}, {1024, 3}, {1280, 2}};
constexpr const LgWidth* lg_width(int K) {
  for (const LgWidth& w : kLgWidths)
    if (w.K == K) return &w;
  return nullptr;
}
// (a width without a kernel sizes its history words as before: 32 rows past 768, else 64)
int logits_row_group(int K) { return lg_width(K) ? lg_width(K)->rows() : K > 768 ? 32 : 64; }
int logits_partial_blocks(int V, int K, int max_blocks) {
  const int cap = max_blocks > 0 ? max_blocks : 256;  // one per CU of a whole MI355X
  return std::max(1, std::min(cap, ((V + 15) / 16 + lg_waves(K) - 1) / lg_waves(K)));
}

// (lse_merge / better: decoder_dev.h, shared with the beam kernels)
// Vocabulary projection + rule-filtered statistics: logits = A[B<=64][K] . W[V][K]^T
// (W = the token embedding, tied). The 53 MB weight read once per step is the cost: each
// block stages A (all rows) in LDS once, then its 8 waves walk 16-column tiles
// independently with the next tile's weight fragments (K/32 x 16 B per lane) and its 16
// suppress-mask bytes in flight during the current tile's epilogue (the first tile's
// during the A staging). A tile's 64 x 16 logits go through a wave-private LDS patch so
// lane = row folds its 16 columns (rule filter, maxima, partition sums, argmaxes) into
// running per-row statistics without shuffles; at the end the 8 waves' statistics are
// merged per row (wave order) into ONE partial per (row, block) for the selector.

// NB: weight tiles in flight per wave. Every launch uses 1: with 2 (two register sets, the
// tile two strides ahead issued after this tile's MFMAs) the decoder side measured 303-305
// vs 302-303 ms per step.
// SAMPLE (decode at temperature > 0, faster-whisper's fallback): the argmaxes are taken
// over the perturbed keys logit * inv_temp + Gumbel noise (Gumbel-max: a draw from
// softmax(logits / T) over the same rule-filtered set), the chosen logit carried beside
// the key for the log-probability; everything else as in the greedy kernel.
// BEAM (beam search, greedy keys): the row's kBeamTop best allowed entries of this block's
// columns ride along (BeamTop: every allowed token / the allowed timestamps), kept per lane
// = row in sorted registers and merged over the 8 waves after the statistics.
// MT: 16-row m-tiles of A per row group (RG = 16 MT rows). 4 up to K = 768: all 64 rows
// of a group in LDS. K = 1280 (the large-v3 family): 64 rows x 1296 halves are 166 KB, more
// than a CU's 160 KB, so a group is 32 rows (MT = 2: 83 KB of A, 17 KB of patches) and lanes
// 32 - 63 idle in the statistics pass; the weights are read once per 32-row group. K = 1024
// (medium.en): 64 rows x 1040 halves + patches + rules are 169 984 B, 6 KB over; 48 rows
// (MT = 3) are 128 000 B and read the table 6 times per 256 rows where MT = 2 reads it 8 times
// (both were timed: DESIGN.md §5q). The LayerNorm prologue is a 64-row-group form only.
// HIST (repetition penalty / no-repeat n-grams, janus_decode_options): the row's history word of
// the tile (history_rules_kernel: bits 0-15 penalised, 16-31 banned columns) arrives with the
// next tile's weights; a penalised column's logit is scaled (x p below 0, / p otherwise)
// before the filter, a banned column fails it like a suppressed token. The raw statistics
// (t_v, m_raw, s_raw) stay on the unpenalised logits; a lane whose word is 0 runs the
// sibling's epilogue unchanged (the plain tile's shortcut included).
// W8 (int8 decoder weights, janus_whisper_set_decoder_compute): W is the int8 table [V][K] and
// wscale its row scales. The tile in flight is NKS x 8 bytes per lane (80 VGPRs at K = 1280
// where the fp16 tile holds 160), converted exactly to fp16 (w8_half8) in front of each MFMA;
// the column's scale arrives with the tile's mask bytes and multiplies the fp32 sums where
// the patch is written: logit = wscale[v] * sum_k a[k] * q[v][k]. Everything after the patch
// is the fp16 form's. No BEAM form.
template <int NKS, int NB, bool SAMPLE, bool BEAM = false, int MT = 4, bool HIST = false, bool W8 = false>  // K / 32
__global__ __launch_bounds__(lg_waves(NKS * 32) * 64) void logits_partial_kernel(
    const _Float16* __restrict__ A, int lda, const _Float16* __restrict__ W, int V, int B,
    DecodeRules R, const uint8_t* __restrict__ smask, const RowRules* __restrict__ rules,
    LogitPart* __restrict__ parts, int ntiles, const float* __restrict__ lnx, int ldx,
    const float* __restrict__ ln_g, const float* __restrict__ ln_b, int rot,
    const uint32_t* __restrict__ seeds, int pos, const float* __restrict__ rinv,
    BeamTop* __restrict__ tops, const uint32_t* __restrict__ hist, float rep_pen,
    const float* __restrict__ wscale) {
  extern __shared__ __attribute__((aligned(16))) _Float16 lg_smem[];
  dec_wave_prio();
  // row group blockIdx.y: rows [RG y, RG y + RG) of the call (one launch for every group:
  // a group's blocks start while the previous group's last blocks drain)
  constexpr int RG = 16 * MT;
  static_assert(!BEAM || MT == 4, "the beam merge is laid out for 64-row groups");
  static_assert(!(HIST && BEAM), "beam search takes no history rules");
  static_assert(!(W8 && BEAM), "the beam partials read the fp16 table only");
  {
    const int r0 = (int)blockIdx.y * RG;
    A += (int64_t)r0 * lda;
    rules += r0;
    parts += (int64_t)r0 * gridDim.x;
    if (lnx) lnx += (int64_t)r0 * ldx;
    if (seeds) seeds += r0;
    if (rinv) rinv += r0;
    if (BEAM) tops += (int64_t)r0 * gridDim.x;
    if constexpr (HIST) hist += (int64_t)blockIdx.y * ntiles * RG;   // [group][tile][RG]
    B = min(RG, B - r0);
  }
  constexpr int K = NKS * 32;
  constexpr int kLgWaves = lg_waves(K);
  constexpr int AP = K + 16;  // row pitch (halves): 16*AP bytes with AP/8 % 4 == 2 -> conflict-free
  _Float16* sA = lg_smem;                                            // [RG][AP]
  float* sT = reinterpret_cast<float*>(sA + RG * AP);                // [waves][RG][17]
  RowRules* sR = reinterpret_cast<RowRules*>(sT + kLgWaves * RG * 17);  // [64]
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  // the first tile's weights and suppress-mask bytes are issued before A is staged (they
  // do not depend on it); later tiles' loads are issued before the previous epilogue
  half8 bw[NB][W8 ? 1 : NKS];
  uint2 bq[NB][W8 ? NKS : 1];   // W8: the tile's int8 weights
  float wsc[NB];                // W8: the scale of column lane & 15 of the tile
  uint4 sm16[NB];
  uint32_t hw[NB];   // HIST: the history word of row = lane for the tile (one coalesced load)
  // logical tile t -> physical tile (t + rot) mod ntiles (see logits_partial_launch)
  auto phys = [&](int t) { const int q = t + rot; return q >= ntiles ? q - ntiles : q; };
#define LG_LOAD(BUF, TILE)                                                                    \
  do {                                                                                        \
    const int bcol_ = min(phys(TILE) * 16 + (lane & 15), V - 1);                              \
    if constexpr (W8) {                                                                       \
      const int8_t* qrow_ = reinterpret_cast<const int8_t*>(W) + (int64_t)bcol_ * K + 8 * (lane >> 4); \
      _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks)                                      \
        bq[BUF][ks] = *reinterpret_cast<const uint2*>(qrow_ + 32 * ks);                       \
      wsc[BUF] = wscale[bcol_];                                                               \
    } else {                                                                                  \
      const _Float16* wrow_ = W + (int64_t)bcol_ * K + 8 * (lane >> 4);                       \
      _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks)                                      \
        bw[BUF][ks] = *reinterpret_cast<const half8*>(wrow_ + 32 * ks);                       \
    }                                                                                         \
    /* 16 mask bytes per tile (the mask buffer is padded to a multiple of 16) */             \
    sm16[BUF] = *reinterpret_cast<const uint4*>(smask + phys(TILE) * 16);                     \
    if constexpr (HIST) hw[BUF] = hist[(int64_t)phys(TILE) * RG + (RG < 64 ? min(lane, RG - 1) : lane)]; \
  } while (0)
  const int tile0 = blockIdx.x * kLgWaves + w;
  const int stride = gridDim.x * kLgWaves;
#pragma unroll
  for (int u = 0; u < NB; ++u)
    if (tile0 + u * stride < ntiles) LG_LOAD(u, tile0 + u * stride);
  bool ln_here = false;
  if constexpr (K <= 1024 && MT == 4) ln_here = lnx != nullptr;  // (ln_rows_wave: d <= 1024; the launcher checks)
  if (ln_here) {  // A = the decoder's final LayerNorm of x, computed here (one wave per row)
    // wave w: rows w + 8j (j < 8), all loads up front
    if constexpr (K <= 1024 && MT == 4)
      ln_rows_wave<(K + 255) / 256, RG / kLgWaves>(lnx, ldx, w, kLgWaves, B, ln_g, ln_b, sA, w, AP, K,
                                                   1e-5f, lane);
  } else {
    for (int i = tid; i < RG * (K / 8); i += kLgWaves * 64) {
      const int r = i / (K / 8), c8 = (i % (K / 8)) * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < B) v = *reinterpret_cast<const uint4*>(A + (int64_t)r * lda + c8);
      *reinterpret_cast<uint4*>(sA + r * AP + c8) = v;
    }
  }
  if constexpr (MT != 4) {
    // (every field set, pad[] too: the half-initialised struct below goes through 12 bytes of
    // scratch per lane, which the instantiations up to K = 768 keep as compiled)
    static_assert(sizeof(RowRules) == 32, "two 16-byte halves");
    if (tid < 64) {   // (rules: 32-byte rows of a device allocation; sR: 16-byte aligned in LDS)
      int4 lo = make_int4(0, 0, 0, -1), hi = make_int4(-1, 0, 0, 0);   // ts_floor, last_stamp: none
      if (tid < B) {
        const int4* src = reinterpret_cast<const int4*>(rules + tid);
        lo = src[0]; hi = src[1];
      }
      int4* dst = reinterpret_cast<int4*>(sR + tid);
      dst[0] = lo; dst[1] = hi;
    }
  } else if (tid < 64) {
    RowRules rr;
    if (tid < B) rr = rules[tid];
    else { rr.sample_begin = 0; rr.suppress_all_ts = rr.suppress_text = 0; rr.ts_floor = -1; rr.last_stamp = -1; }
    sR[tid] = rr;
  }
  __syncthreads();
  float* patch = sT + w * RG * 17;
  const int lr = lane & 15, kc8 = 8 * (lane >> 4);
  RowRules rr;  // lane = row in the statistics pass (fields copied: no scratch for pad[])
  rr.sample_begin = sR[lane].sample_begin; rr.suppress_all_ts = sR[lane].suppress_all_ts;
  rr.suppress_text = sR[lane].suppress_text; rr.ts_floor = sR[lane].ts_floor;
  // this row's 1 / T (sampling): per row when the call mixes temperatures; 0 = a greedy
  // row (key = logit, as the greedy kernel)
  const float inv_t = SAMPLE && rinv ? rinv[min(lane, B - 1)] : R.inv_temp;
  // running statistics of this wave's tiles for row = lane
  float m_all = -INFINITY, s_all = 0.f, m_text = -INFINITY, m_ts = -INFINITY, s_ts = 0.f;
  float ba_v = -INFINITY, bt_v = -INFINITY;
  int ba_i = 0x7fffffff, bt_i = 0x7fffffff;
  float m_raw = -INFINITY, s_raw = 0.f, t_v = -INFINITY;  // unfiltered softmax, target logit
  float ba_r = -INFINITY, bt_r = -INFINITY;                // logits of the sampled argmaxes
  uint32_t nb = 0;                                         // row's noise base at this position
  if constexpr (SAMPLE) nb = noise_base(lane < B ? seeds[lane] : 0u, pos);
  // BEAM: sorted best lists of row = lane (static indices only: they stay in registers)
  float la_v[kBeamTop], lt_v[kBeamTop];
  int la_i[kBeamTop], lt_i[kBeamTop];
  if constexpr (BEAM) {
#pragma unroll
    for (int q = 0; q < kBeamTop; ++q) { la_v[q] = lt_v[q] = -INFINITY; la_i[q] = lt_i[q] = 0x7fffffff; }
  }
  auto beam_ins = [&](float (&lv)[kBeamTop], int (&li)[kBeamTop], float v, int t)
      __attribute__((always_inline)) {
    if (!better(v, t, lv[kBeamTop - 1], li[kBeamTop - 1])) return;
#pragma unroll
    for (int q = 0; q < kBeamTop; ++q) {
      const bool bt = better(v, t, lv[q], li[q]);
      const float ov = lv[q];
      const int oi = li[q];
      lv[q] = bt ? v : ov; li[q] = bt ? t : oi;
      v = bt ? ov : v; t = bt ? oi : t;
    }
  };
  for (int tb = tile0; tb < ntiles; tb += NB * stride) {
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int tile = tb + u * stride;
    if (tile >= ntiles) break;  // wave-uniform
    const int col0 = phys(tile) * 16;
    f32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = zero_f32x4();
    // A fragments of k-step ks+1 read while k-step ks's MFMAs run (left to the compiler,
    // every ds_read was followed by an lgkmcnt(0) wait and one MFMA: 64 exposed LDS round
    // trips per tile)
    half8 af[2][MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) af[0][m] = *reinterpret_cast<const half8*>(sA + (16 * m + lr) * AP + kc8);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (ks + 1 < NKS) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
          af[(ks + 1) & 1][m] = *reinterpret_cast<const half8*>(sA + (16 * m + lr) * AP + 32 * (ks + 1) + kc8);
      }
      // keep the reads above the MFMAs (the scheduler otherwise sinks each read to just
      // before its MFMA to save registers, re-serialising the loop)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (W8) {
        const half8 bh = w8_half8(bq[u][ks]);
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mfma16(af[ks & 1][m], bh, acc[m]);
      } else {
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = mfma16(af[ks & 1][m], bw[u][ks], acc[m]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (W8) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[m][r] *= wsc[u];
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) patch[(16 * m + 4 * (lane >> 4) + r) * 17 + lr] = acc[m][r];
    const uint4 smc = sm16[u];
    uint32_t hwd = 0;
    if constexpr (HIST) hwd = hw[u];
    // a penalised column's logit (rule 1 of janus_decode_options), fp32
    auto penal = [&](float v) { return v < 0.f ? v * rep_pen : v / rep_pen; };
    // the tile NB strides ahead into the registers just consumed, during the epilogue
    if (tile + NB * stride < ntiles) LG_LOAD(u, tile + NB * stride);
    // wave-private patch: the wave's own stores are visible to its loads in order
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    const int row = lane;
    const int prow = RG < 64 ? min(row, RG - 1) : row;  // lanes past the group read its last row (unused)
    float t_all = -INFINITY, t_text = -INFINITY, t_ts = -INFINITY, t_raw = -INFINITY;
    float vals[16];
    unsigned okm = 0;
    float u_all = 0.f, u_ts = 0.f, u_raw = 0.f;
    auto in_tile = [&](int t) { return t >= col0 && t < col0 + 16; };
    // Plain tile (wave-uniform): 16 in-vocabulary text or special tokens, none of blank /
    // eot / no_timestamps, no timestamp: the rules then give one verdict per row for the
    // whole tile (allowed_unmasked reduces to the row flags below), and when every column
    // is allowed the filtered softmax sum IS the raw one (same maximum, same terms in the
    // same order) — half the exponentials. Bit-identical to the general path.
    const bool plain = col0 + 16 <= V && (R.ts_begin < 0 || col0 + 16 <= R.ts_begin) &&
                       !in_tile(R.blank) && !in_tile(R.eot) && !in_tile(R.no_timestamps);
    if (plain) {
      const bool row_ok = row < B && !(R.ts_begin >= 0 && ((rr.suppress_text && col0 < R.eot) || rr.sample_begin));
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float v = patch[prow * 17 + c];
        vals[c] = v;
        t_raw = fmaxf(t_raw, v);
        if (col0 + c == R.target) t_v = v;
        const unsigned smw = c < 4 ? smc.x : c < 8 ? smc.y : c < 12 ? smc.z : smc.w;
        bool ok = row_ok && !((smw >> (8 * (c & 3))) & 0xffu);
        float pv = v;
        if constexpr (HIST) {
          ok = ok && !((hwd >> (16 + c)) & 1u);
          if ((hwd >> c) & 1u) pv = penal(v);
        }
        okm |= (unsigned)ok << c;
        if (ok) t_all = fmaxf(t_all, pv);
      }
      t_text = t_all;
#pragma unroll
      for (int c = 0; c < 16; ++c) u_raw += __expf(vals[c] - t_raw);
      bool full = okm == 0xffffu;
      if constexpr (HIST) {   // the raw sum is done: the penalised logits take its registers
        if (hwd & 0xffffu) {
          full = false;
#pragma unroll
          for (int c = 0; c < 16; ++c)
            if ((hwd >> c) & 1u) vals[c] = penal(vals[c]);
        }
      }
      if (full) {
        u_all = u_raw;
      } else {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if ((okm >> c) & 1u) u_all += __expf(vals[c] - t_all);
      }
      if constexpr (SAMPLE) {
        for (int c = 0; c < 16; ++c) {
          if (!((okm >> c) & 1u)) continue;
          const float key = inv_t > 0.f ? vals[c] * inv_t + sample_gumbel(nb, col0 + c) : vals[c];
          if (better(key, col0 + c, ba_v, ba_i)) { ba_v = key; ba_i = col0 + c; ba_r = vals[c]; }
        }
      } else {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (((okm >> c) & 1u) && better(vals[c], col0 + c, ba_v, ba_i)) { ba_v = vals[c]; ba_i = col0 + c; }
        if constexpr (BEAM) {
#pragma unroll
          for (int c = 0; c < 16; ++c)
            if ((okm >> c) & 1u) beam_ins(la_v, la_i, vals[c], col0 + c);
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const int t = col0 + c;
        const float v = patch[prow * 17 + c];
        vals[c] = v;
        if (t < V) t_raw = fmaxf(t_raw, v);
        if (t == R.target) t_v = v;
        const unsigned smw = c < 4 ? smc.x : c < 8 ? smc.y : c < 12 ? smc.z : smc.w;
        const bool masked = (smw >> (8 * (c & 3))) & 0xffu;
        bool ok = row < B && t < V && !masked && allowed_unmasked(t, R, rr, false);
        float pv = v;
        if constexpr (HIST) {
          ok = ok && !((hwd >> (16 + c)) & 1u);
          if ((hwd >> c) & 1u) pv = penal(v);
        }
        okm |= (unsigned)ok << c;
        if (ok) {
          t_all = fmaxf(t_all, pv);
          if (R.ts_begin >= 0 && t >= R.ts_begin) t_ts = fmaxf(t_ts, pv);
          else t_text = fmaxf(t_text, pv);
        }
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) u_raw += (col0 + c < V) ? __expf(vals[c] - t_raw) : 0.f;
      if constexpr (HIST) {
        if (hwd & 0xffffu) {
#pragma unroll
          for (int c = 0; c < 16; ++c)
            if ((hwd >> c) & 1u) vals[c] = penal(vals[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        if (!((okm >> c) & 1u)) continue;
        const int t = col0 + c;
        const float v = vals[c];
        u_all += __expf(v - t_all);
        // sampling: the key (perturbed logit) is compared, the logit kept beside it
        const float key = SAMPLE && inv_t > 0.f ? v * inv_t + sample_gumbel(nb, t) : v;
        if (better(key, t, ba_v, ba_i)) { ba_v = key; ba_i = t; ba_r = v; }
        if constexpr (BEAM) beam_ins(la_v, la_i, v, t);
        if (R.ts_begin >= 0 && t >= R.ts_begin) {
          u_ts += __expf(v - t_ts);
          if (better(key, t, bt_v, bt_i)) { bt_v = key; bt_i = t; bt_r = v; }
          if constexpr (BEAM) beam_ins(lt_v, lt_i, v, t);
        }
      }
    }
    float mo;
    s_all = lse_merge(m_all, s_all, t_all, u_all, &mo); m_all = mo;
    s_ts = lse_merge(m_ts, s_ts, t_ts, u_ts, &mo); m_ts = mo;
    s_raw = lse_merge(m_raw, s_raw, t_raw, u_raw, &mo); m_raw = mo;
    m_text = fmaxf(m_text, t_text);
  }
  }
  // merge the 8 waves' statistics per row (wave order), one partial per (row, block)
  __syncthreads();  // every wave is done with its patch: reuse sT for the wave partials
  LogitPart* wp = reinterpret_cast<LogitPart*>(sT);  // [kLgWaves][RG]
  static_assert(sizeof(LogitPart) <= 17 * 4, "the wave partials fit the patches");
  if (lane < RG) {
    LogitPart p;
    p.m_all = m_all; p.s_all = s_all; p.m_text = m_text; p.m_ts = m_ts; p.s_ts = s_ts;
    p.b_all_v = ba_v; p.b_all_i = ba_i; p.b_ts_v = bt_v; p.b_ts_i = bt_i;
    p.b_all_r = SAMPLE ? ba_r : ba_v; p.b_ts_r = SAMPLE ? bt_r : bt_v;
    p.t_v = t_v; p.m_raw = m_raw; p.s_raw = s_raw;
    wp[w * RG + lane] = p;
  }
  __syncthreads();
  if (w == 0 && lane < B) {
    LogitPart q = wp[lane];
    for (int k = 1; k < kLgWaves; ++k) {
      const LogitPart p = wp[k * RG + lane];
      float mo;
      q.s_all = lse_merge(q.m_all, q.s_all, p.m_all, p.s_all, &mo); q.m_all = mo;
      q.s_ts = lse_merge(q.m_ts, q.s_ts, p.m_ts, p.s_ts, &mo); q.m_ts = mo;
      q.m_text = fmaxf(q.m_text, p.m_text);
      if (better(p.b_all_v, p.b_all_i, q.b_all_v, q.b_all_i)) { q.b_all_v = p.b_all_v; q.b_all_i = p.b_all_i; q.b_all_r = p.b_all_r; }
      if (better(p.b_ts_v, p.b_ts_i, q.b_ts_v, q.b_ts_i)) { q.b_ts_v = p.b_ts_v; q.b_ts_i = p.b_ts_i; q.b_ts_r = p.b_ts_r; }
      q.s_raw = lse_merge(q.m_raw, q.s_raw, p.m_raw, p.s_raw, &mo); q.m_raw = mo;
      q.t_v = fmaxf(q.t_v, p.t_v);
    }
    parts[(int64_t)lane * gridDim.x + blockIdx.x] = q;
  }
  if constexpr (BEAM) {
    // the 8 waves' sorted lists of each row -> the block's best kBeamTop, one set at a time
    // through LDS ([wave][slot][row]: 64 KB over the A tile and the patches, both done with)
    float* mv = reinterpret_cast<float*>(lg_smem);
    int* mi = reinterpret_cast<int*>(mv + kLgWaves * kBeamTop * 64);
    BeamTop* dst = tops + (int64_t)lane * gridDim.x + blockIdx.x;
#pragma unroll
    for (int set = 0; set < 2; ++set) {
      __syncthreads();  // the previous user of this LDS (wave partials / the other set) is done
#pragma unroll
      for (int q = 0; q < kBeamTop; ++q) {
        mv[(w * kBeamTop + q) * 64 + lane] = set ? lt_v[q] : la_v[q];
        mi[(w * kBeamTop + q) * 64 + lane] = set ? lt_i[q] : la_i[q];
      }
      __syncthreads();
      if (w == 0 && lane < B) {
        float hv[kLgWaves];
        int hi[kLgWaves], hp[kLgWaves];
#pragma unroll
        for (int k = 0; k < kLgWaves; ++k) {
          hp[k] = 0;
          hv[k] = mv[(k * kBeamTop) * 64 + lane];
          hi[k] = mi[(k * kBeamTop) * 64 + lane];
        }
        for (int q = 0; q < kBeamTop; ++q) {
          float bv = hv[0];
          int bi = hi[0], bk = 0;
#pragma unroll
          for (int k = 1; k < kLgWaves; ++k)
            if (better(hv[k], hi[k], bv, bi)) { bv = hv[k]; bi = hi[k]; bk = k; }
          if (set) { dst->tv[q] = bv; dst->ti[q] = bi; }
          else { dst->av[q] = bv; dst->ai[q] = bi; }
#pragma unroll
          for (int k = 0; k < kLgWaves; ++k)
            if (k == bk) {
              hp[k] += 1;
              const bool in = hp[k] < kBeamTop;
              const int o = (k * kBeamTop + (in ? hp[k] : 0)) * 64 + lane;
              hv[k] = in ? mv[o] : -INFINITY;
              hi[k] = in ? mi[o] : 0x7fffffff;
            }
        }
      }
    }
  }
}
#undef LG_LOAD

// The projection's kernel by its key (width, SAMPLE, BEAM, HIST, W8). Every instantiation has
// the same parameters, so one function type; each travels with its own LDS opt-in.
using LgKernel = LdsKernel<decltype(logits_partial_kernel<12, 1, false>)>;

// The forms built: the beam partials are greedy, on the fp16 table, without history rules and
// laid out for 64-row groups (the kernel's static_asserts); every other combination exists.
constexpr bool lg_built(LgWidth w, bool sample, bool beam, bool hist, bool w8) {
  return !beam || (w.MT == 4 && !sample && !hist && !w8);
}

template <int WI, bool SAMPLE, bool BEAM, bool HIST, bool W8>
constexpr LgKernel lg_select() {
  constexpr LgWidth w = kLgWidths[WI];
  if constexpr (lg_built(w, SAMPLE, BEAM, HIST, W8))
    return lds_kernel<logits_partial_kernel<w.nks(), 1, SAMPLE, BEAM, w.MT, HIST, W8>>();
  else
    return {nullptr, nullptr};
}
// From run-time flags to template arguments, one flag per step: lg_select<WI>(s, b, h, q) calls
// lg_select<WI, s>(b, h, q), ... until no flag is left and the overload above, which takes all
// four as template arguments and none as parameters, is the only one that matches.
template <int WI, bool... Fs, class... Rest>
constexpr LgKernel lg_select(bool flag, Rest... rest) {
  return flag ? lg_select<WI, Fs..., true>(rest...) : lg_select<WI, Fs..., false>(rest...);
}

// (the row of kLgWidths with this K, whichever rows the list holds; no row: no kernel)
template <size_t... WI>
constexpr LgKernel lg_kernel(int K, bool sample, bool beam, bool hist, bool w8, std::index_sequence<WI...>) {
  LgKernel k{nullptr, nullptr};
  ((kLgWidths[WI].K == K ? (void)(k = lg_select<(int)WI>(sample, beam, hist, w8)) : (void)0), ...);
  return k;
}
constexpr LgKernel lg_kernel(int K, bool sample, bool beam, bool hist, bool w8) {
  return lg_kernel(K, sample, beam, hist, w8, std::make_index_sequence<sizeof(kLgWidths) / sizeof(kLgWidths[0])>{});
}

// the table holds exactly the forms the launcher has always had: counted by part of the key
constexpr int lg_count(int k_lo, int k_hi, int beam, int hist, int w8) {   // (-1: either)
  int n = 0;
  for (const LgWidth& w : kLgWidths)
    for (int f = 0; f < 16; ++f) {
      const bool s = f & 1, b = f & 2, h = f & 4, q = f & 8;
      if (w.K < k_lo || w.K > k_hi || (beam >= 0 && b != (beam != 0)) || (hist >= 0 && h != (hist != 0)) ||
          (w8 >= 0 && q != (w8 != 0)))
        continue;
      n += lg_kernel(w.K, s, b, h, q).fn != nullptr;
    }
  return n;
}
static_assert(lg_count(384, 768, -1, 0, 0) == 9, "3 widths x {greedy, sample, beam}");
static_assert(lg_count(1024, 1280, -1, 0, 0) == 4, "1024 and 1280 x {greedy, sample}");
static_assert(lg_count(384, 1280, -1, 1, 0) == 10, "5 widths x {greedy, sample} with HIST");
static_assert(lg_count(384, 1280, -1, -1, 1) == 20, "5 x 2 x 2 with W8");
static_assert(lg_count(384, 1280, -1, -1, -1) == 43, "the forms of logits_partial_kernel");

void logits_partial_launch(const LogitsArgs& a, hipStream_t s) {
  const DecodeRules& R = a.R;
  const int K = a.K, V = a.V, B = a.B;
  JANUS_CHECK(!a.tops || !(R.inv_temp > 0.f), "logits: the beam partials are greedy only");
  JANUS_CHECK(!a.Wq || (a.wscale && !a.tops && !a.lnx && ((uintptr_t)a.Wq & 7) == 0),
              "logits: the int8 table needs its row scales and has no beam partials and no LayerNorm prologue");
  JANUS_CHECK(!a.hist || (!a.tops && a.rep_pen > 0.f), "logits: history rules need a penalty > 0 and no beam partials");
  const LgWidth* w = lg_width(K);
  JANUS_CHECK(w != nullptr, "logits: K (d_model) must be 384, 512, 768, 1024 or 1280");
  // K = 1024 / 1280: 48- / 32-row groups (64 rows of A do not fit a CU's LDS), greedy and sampling only
  JANUS_CHECK(w->MT == 4 || (!a.tops && !a.lnx),
              "logits: K = 1024 / 1280 has no beam partials and no LayerNorm prologue");
  const bool sample = R.inv_temp > 0.f;
  JANUS_CHECK(!sample || a.seeds, "logits: sampling needs per-row seeds");
  const LgKernel kern = lg_kernel(K, sample, a.tops != nullptr, a.hist != nullptr, a.Wq != nullptr);
  JANUS_CHECK(kern.fn != nullptr, "logits: no kernel of this form");   // (the refusals above leave none)
  kern.allow(160 * 1024);
  const int ntiles = (V + 15) / 16;
  const int nw = lg_waves(K), rg = w->rows();
  const int grid = logits_partial_blocks(V, K, a.max_blocks);
  // Tile rotation: waves take tiles t, t + stride, ...; the first ntiles % stride waves get
  // one tile more and set the kernel's length. The special tiles (eot / no_timestamps /
  // timestamps at the top of the vocabulary, and the blank token's tile) run the general
  // rule-filter epilogue, several times a plain tile's VALU work; rotated so they land in
  // the first round of the waves with one tile fewer. Order-dependent only in the last
  // bits of the softmax sums (the argmax ties break by index either way).
  int rot = 0;
  {
    const int stride = grid * nw, rem = ntiles % stride;
    int s0 = ntiles;
    for (int t : {R.eot, R.no_timestamps, R.ts_begin})
      if (t >= 0 && t < V) s0 = std::min(s0, t / 16);
    const int nspec = ntiles - s0;
    if (rem > 0 && nspec > 0 && rem + nspec + (R.blank >= 0 ? 1 + R.blank / 16 : 0) <= stride)
      rot = ((s0 - rem) % ntiles + ntiles) % ntiles;
  }
  // the int8 forms read their table through the fp16 table's parameter
  const _Float16* table = a.Wq ? reinterpret_cast<const _Float16*>(a.Wq) : a.W;
  // 64 (K = 1024: 48, K = 1280: 32) rows per row group (blockIdx.y), every group in one launch
  auto* fn = kern.fn;
  fn<<<dim3(grid, (B + rg - 1) / rg), nw * 64, w->lds(), s>>>(a.A, a.lda, table, V, B, R, a.smask, a.rules, a.parts,
                                                            ntiles, a.lnx, a.ldx, a.ln_g, a.ln_b, rot, a.seeds,
                                                            a.pos, sample ? a.row_inv_temp : nullptr, a.tops,
                                                            a.hist, a.rep_pen, a.wscale);
  JANUS_LAUNCH_CHECK();
}

// ------------------------------------------------------- row history (HIST logits kernel)
// The history words of one row at position pos, from the tokens it has sampled in this call,
// g = tokens[plen .. pos] (m = pos + 1 - plen of them): hist [group][tile][rg] uint32, row b in
// group b / rg, bits 0-15 of a word the penalised columns of the 16-column tile, 16-31 the
// banned ones (rule of janus_decode_options). One block per row, launched once per position in
// front of the vocabulary projection: the token at pos joins the penalised set; the bans of
// position pos - 1 (recomputed from g without its last token) are cleared, then those of pos
// set: every start i <= m - n whose n - 1 tokens equal the last n - 1 of g bans g[i + n - 1]
// (n = 1: every token of g). A row inside its prompt does nothing.
__global__ __launch_bounds__(256) void history_rules_kernel(
    const int32_t* __restrict__ tokens, int ld, int pos, const int32_t* __restrict__ plen, int n, int V,
    int ntiles, int rg, uint32_t* __restrict__ hist) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int pl = plen[b];
  const int m = pos + 1 - pl;
  if (m <= 0 || pos >= ld) return;  // block-uniform
  const int32_t* g = tokens + (int64_t)b * ld + pl;
  uint32_t* words = hist + (int64_t)(b / rg) * ntiles * rg + (b % rg);
  auto word = [&](int t) { return words + (int64_t)(t >> 4) * rg; };
  if (tid == 0) {
    const int t = g[m - 1];
    if (t >= 0 && t < V) atomicOr(word(t), 1u << (t & 15));
  }
  if (n <= 0) return;
  // the bans of a history of mm tokens, set or cleared
  auto bans = [&](int mm, bool set) {
    for (int i = tid; i + n <= mm; i += blockDim.x) {
      bool eq = true;
      for (int j = 0; j + 1 < n; ++j) eq = eq && g[i + j] == g[mm - n + 1 + j];
      const int t = g[i + n - 1];
      if (!eq || t < 0 || t >= V) continue;
      if (set) atomicOr(word(t), 0x10000u << (t & 15));
      else atomicAnd(word(t), ~(0x10000u << (t & 15)));
    }
  };
  bans(m - 1, false);
  __syncthreads();  // (every clear issued and complete before a set of the same word)
  bans(m, true);
}

void history_rules_launch(const int32_t* tokens, int ld, int pos, const int32_t* plen, int n, int V,
                          int rg, uint32_t* hist, int B, hipStream_t s) {
  JANUS_CHECK(tokens && plen && hist, "history_rules: null argument");
  JANUS_CHECK(B >= 1 && n >= 0 && V >= 1 && pos >= 0 && pos < ld && (rg == 32 || rg == 48 || rg == 64),
              "history_rules: need B >= 1, n >= 0, 0 <= pos < ld, row groups of 32, 48 or 64");
  history_rules_kernel<<<B, 256, 0, s>>>(tokens, ld, pos, plen, n, V, (V + 15) / 16, rg, hist);
  JANUS_LAUNCH_CHECK();
}

size_t history_words(int V, int K, int B) {
  const int rg = logits_row_group(K);
  return (size_t)((B + rg - 1) / rg) * ((V + 15) / 16) * rg;
}


// One block per row: reduce the partials, apply the timestamp-probability rule, pick
// the token, accumulate its log-probability and derive the next step's row rules.
// Row b's selection at position pos; returns (in thread 0) the row's token at pos + 1:
// the selected one, eot for a finished row, the forced one inside the row's prompt.
// roff (nullable): per-row position offsets (staggered rows, janus_decode_rows.pos_offset):
// row b is at position pos + roff[b]; a row whose next position would pass the token
// buffer (pos + 1 >= ld) has finished and writes nothing (returns -1).
__device__ __forceinline__ int select_row(
    const LogitPart* __restrict__ parts, int nblk, const DecodeRules& R, RowRules* __restrict__ rules,
    int32_t* __restrict__ tokens, int ld, int pos, int32_t* __restrict__ done,
    float* __restrict__ sum_lp, int32_t* __restrict__ n_tok, const int32_t* __restrict__ plen,
    float* __restrict__ nsp, const int32_t* __restrict__ roff = nullptr) {
  __shared__ LogitPart sh[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (roff) {
    pos += roff[b];
    if (pos + 1 >= ld) return -1;  // block-uniform
  }
  int32_t* row_tok = tokens + (int64_t)b * ld;
  const int pl = plen ? plen[b] : 1;
  if (pos + 1 < pl) {  // inside this row's prompt: the forced token stays
    // no_speech_prob read before the prompt's end (the <|startoftranscript|> position of a
    // [sot, language, task] prompt): the raw statistics alone, no rule state, counter or
    // token touched (block-uniform: pos, pl and R are)
    if (nsp && pos + 1 + R.target_back == pl) {
      const LogitPart q = row_parts_reduce(parts + (int64_t)b * nblk, nblk, sh);
      if (tid == 0) nsp[b] = R.target >= 0 ? __expf(q.t_v - (q.m_raw + __logf(q.s_raw))) : 0.f;
    }
    return row_tok[pos + 1];
  }
  if (done[b]) {
    if (tid == 0) row_tok[pos + 1] = R.eot;
    return R.eot;
  }
  // the row's partials merged (decoder_dev.h: the same reduction the beam step runs)
  const LogitPart q = row_parts_reduce(parts + (int64_t)b * nblk, nblk, sh);
  if (tid != 0) return -1;
  const float m_all = q.m_all, s_all = q.s_all, m_text = q.m_text, m_ts = q.m_ts, s_ts = q.s_ts;
  const float m_raw = q.m_raw, s_raw = q.s_raw, t_v = q.t_v, ba_r = q.b_all_r, bt_r = q.b_ts_r;
  const int ba_i = q.b_all_i, bt_i = q.b_ts_i;
  // no_speech_prob: the raw softmax probability of the target token at the row's first
  // sampled step (logits at the <|startoftranscript|> position, before any filter)
  if (nsp && pos + 1 + R.target_back == pl) nsp[b] = R.target >= 0 ? __expf(t_v - (m_raw + __logf(s_raw))) : 0.f;
  const float lse_all = m_all + __logf(s_all);
  // the chosen token's log-probability uses its logit (b_*_r; = the key when greedy)
  int next = ba_i;
  float lp = ba_r - lse_all;
  if (R.ts_begin >= 0 && m_ts > -INFINITY) {
    const float lse_ts = m_ts + __logf(s_ts);
    if (lse_ts - lse_all > m_text - lse_all) {  // timestamp mass beats every text token
      next = bt_i;
      lp = bt_r - lse_ts;
    }
  }
  row_tok[pos + 1] = next;
  sum_lp[b] += lp;
  n_tok[b] += 1;
  if (next == R.eot) done[b] = 1;
  // rules for the next step
  rules[b] = next_row_rules(rules[b], R, row_tok[pos], next);
  return next;
}

__global__ __launch_bounds__(256) void select_partials_kernel(
    const LogitPart* __restrict__ parts, int nblk, DecodeRules R, RowRules* __restrict__ rules,
    int32_t* __restrict__ tokens, int ld, int pos, int32_t* __restrict__ done,
    float* __restrict__ sum_lp, int32_t* __restrict__ n_tok, const int32_t* __restrict__ plen,
    float* __restrict__ nsp, const int32_t* __restrict__ roff) {
  (void)select_row(parts, nblk, R, rules, tokens, ld, pos, done, sum_lp, n_tok, plen, nsp, roff);
}

// The selection at position pos and the embedding of the chosen token at pos + 1 in one
// launch (both are per row: one block per utterance): one launch per position fewer.
// Bit-identical to select_partials_kernel followed by embed_kernel at pos + 1.
__global__ __launch_bounds__(256) void select_embed_kernel(
    const LogitPart* __restrict__ parts, int nblk, DecodeRules R, RowRules* __restrict__ rules,
    int32_t* __restrict__ tokens, int ld, int pos, int32_t* __restrict__ done,
    float* __restrict__ sum_lp, int32_t* __restrict__ n_tok, const int32_t* __restrict__ plen,
    float* __restrict__ nsp, const _Float16* __restrict__ tok_emb, const float* __restrict__ pos_emb,
    int d, float* __restrict__ x, float2* __restrict__ part, const float* __restrict__ ln_g,
    const float* __restrict__ ln_b, _Float16* __restrict__ ln_out, const int32_t* __restrict__ roff) {
  __shared__ int s_tok;
  dec_wave_prio();
  const int t = select_row(parts, nblk, R, rules, tokens, ld, pos, done, sum_lp, n_tok, plen, nsp, roff);
  const int pb = pos + (roff ? roff[blockIdx.x] : 0);
  if (pb + 1 >= ld) return;  // a staggered row past its last position: nothing to embed
  if (threadIdx.x == 0) s_tok = t;
  __syncthreads();
  embed_row(tok_emb, pos_emb, s_tok, blockIdx.x, pb + 1, d, x, part, ln_g, ln_b, ln_out);
}

void select_embed_launch(const SelectArgs& a, int B, hipStream_t s, const _Float16* tok_emb,
                         const float* pos_emb, int d, float* x, float2* part, const float* ln_g,
                         const float* ln_b, _Float16* ln_out) {
  JANUS_CHECK(d % 16 == 0, "embed: d % 16 != 0");
  JANUS_CHECK(!ln_out || d <= 512, "embed: fused LayerNorm needs d <= 512");
  select_embed_kernel<<<B, 256, 0, s>>>(a.parts, a.nblk, a.R, a.rules, a.tokens, a.ld, a.pos, a.done, a.sum_lp,
                                        a.n_tok, a.plen, a.nsp, tok_emb, pos_emb, d, x, part, ln_g, ln_b,
                                        ln_out, a.roff);
  JANUS_LAUNCH_CHECK();
}

void select_partials_launch(const SelectArgs& a, int B, hipStream_t s) {
  select_partials_kernel<<<B, 256, 0, s>>>(a.parts, a.nblk, a.R, a.rules, a.tokens, a.ld, a.pos, a.done,
                                           a.sum_lp, a.n_tok, a.plen, a.nsp, a.roff);
  JANUS_LAUNCH_CHECK();
}

// The sampling noise the SAMPLE logits kernel adds, written out (kernel-level ABI
// janus_sample_gumbel_f32: the CPU oracle's restatement is checked against it)
__global__ void sample_gumbel_kernel(const uint32_t* __restrict__ seeds, int pos, int V,
                                     float* __restrict__ out) {
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < V) out[(int64_t)b * V + t] = sample_gumbel(noise_base(seeds[b], pos), t);
}

void sample_gumbel_launch(const uint32_t* seeds, int B, int pos, int V, float* out, hipStream_t s) {
  JANUS_CHECK(B >= 1 && V >= 1, "sample_gumbel: empty shape");
  sample_gumbel_kernel<<<dim3((unsigned)cdiv(V, 256), (unsigned)B), 256, 0, s>>>(seeds, pos, V, out);
  JANUS_LAUNCH_CHECK();
}

void build_mask_launch(const int32_t* list, int n, uint8_t* mask, int V, hipStream_t s) {
  JANUS_HIP(hipMemsetAsync(mask, 0, V, s));
  if (n > 0) {
    build_mask_kernel<<<(n + 255) / 256, 256, 0, s>>>(list, n, mask, V);
    JANUS_LAUNCH_CHECK();
  }
}

}  // namespace janus

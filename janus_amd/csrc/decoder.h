// Decoder-loop kernels (decoder.hip).
#pragma once
#include "common.h"
#include "decode_shapes.h"  // DecodeRules, kBeamMax

namespace janus {

// Per-row rule state carried across steps (computed by the selector for the next step).
struct RowRules {
  int sample_begin;       // no token sampled yet
  int suppress_all_ts;    // last two sampled were timestamps
  int suppress_text;      // last was a timestamp, penultimate was not: text (< eot) banned
  int ts_floor;           // timestamps < ts_floor banned (-1: none)
  int last_stamp;         // last sampled timestamp token (-1: none)
  int pad[3];
};

// Per (row, 16-column block) partial statistics of the rule-filtered logits.
struct LogitPart {
  float m_all, s_all;     // max / sum exp(v - m_all) over allowed tokens
  float m_text;           // max over allowed text tokens (< ts_begin)
  float m_ts, s_ts;       // max / sum exp over allowed timestamp tokens
  float b_all_v; int b_all_i;  // argmax over allowed (first index on ties); sampling: of the
                               // perturbed key logit * inv_temp + gumbel
  float b_ts_v; int b_ts_i;    // the same over allowed timestamps
  float t_v;              // raw logit of DecodeRules::target (-inf if not in this block)
  float m_raw, s_raw;     // max / sum exp over ALL tokens (unfiltered softmax)
  float b_all_r, b_ts_r;  // the logits of b_all_i / b_ts_i (= b_*_v when greedy)
};

// Beam search: per (row, block) the best kBeamTop allowed entries of the block's columns
// beside its LogitPart, sorted (logit descending, first index on ties); unused slots hold
// (-inf, 0x7fffffff). Two sets, because which applies is known only once the whole row's
// timestamp-mass rule is evaluated: every allowed token / the allowed timestamps.
constexpr int kBeamTop = 16;    // 2 * the largest beam size (kBeamMax)
struct BeamTop {
  float av[kBeamTop]; int ai[kBeamTop];
  float tv[kBeamTop]; int ti[kBeamTop];
};

// Sampling noise (decode at temperature > 0): a counter-based hash of (row seed, position,
// token), so a row's draws do not depend on its batch neighbours or the tile schedule and
// the CPU oracle can regenerate them (oracle/whisper.py sample_noise).
__host__ __device__ inline uint32_t noise_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__host__ __device__ inline uint32_t noise_base(uint32_t seed, int pos) {
  return noise_mix(seed ^ noise_mix((uint32_t)pos * 0x9e3779b9u + 0x7f4a7c15u));
}
// uniform u = an odd multiple of 2^-24 in (0, 1), exact in f32; Gumbel(0, 1) = -log(-log u)
__device__ inline float sample_gumbel(uint32_t base, int token) {
  const uint32_t h = noise_mix(base ^ ((uint32_t)token * 0x27d4eb2fu));
  const float u = (float)((h >> 8) | 1u) * 0x1p-24f;
  return -logf(-logf(u));
}

void cast_f16_f32_launch(const _Float16* in, float* out, int64_t n, hipStream_t s);
void cast_f32_f16_launch(const float* in, _Float16* out, int64_t n, hipStream_t s);
// x[b] = tok_emb[token] + pos_emb[pos]; part (nullable): LayerNorm pieces of x
// (SkinnyLnArgs), d % 16 == 0
// x[b] = tok_emb[token] + pos_emb[pos]; optionally the first layer's LayerNorm of the
// row into ln_out [B][d] fp16 (d <= 512, eps 1e-5).
// roff (nullable, device int32 [B]): per-row position offsets — row b is at pos + roff[b]
// (staggered decode: janus_decode_rows.pos_offset)
void embed_launch(const _Float16* tok_emb, const float* pos_emb, const int32_t* tokens,
                  int ld_tokens, int pos, int d, float* x, float2* part, int B, hipStream_t s,
                  const float* ln_g = nullptr, const float* ln_b = nullptr,
                  _Float16* ln_out = nullptr, const int32_t* roff = nullptr);
void kv_store_launch(const _Float16* qkv, int d, int pos, int n_ctx, _Float16* kc, _Float16* vc,
                     int B, hipStream_t s);
void init_tokens_launch(int32_t* tokens, int ld, const int32_t* prompt, int plen, int32_t* done,
                        float* sum_lp, int32_t* n_tok, int B, hipStream_t s);
// per-row prompts: tokens [B][ld] arrive pre-filled (prompt, then -1); only the counters reset
void init_counters_launch(int32_t* done, float* sum_lp, int32_t* n_tok, float* nsp, int B,
                          hipStream_t s);
void select_launch(const float* logits, int V, const DecodeRules& R, const uint8_t* smask,
                   int32_t* tokens, int ld, int pos, int sample_begin_pos, int32_t* done,
                   float* sum_lp, int32_t* n_tok, int B, hipStream_t s);
void rules_init_launch(RowRules* rules, int B, hipStream_t s);
// logits = A[B][K] . W[V][K]^T computed block-wise with the filtered statistics reduced
// in the epilogue (no logits in HBM); nblk = logits_partial_blocks(V) merged partials per row
// (one per block of the launch).
int logits_partial_blocks(int V, int K, int max_blocks = 256);
// rows of A one block holds in LDS (the weights are read once per group of that many rows):
// 64 up to K = 768, 48 at K = 1024, 32 at K = 1280
int logits_row_group(int K);
// The kernel form follows from the fields set: R.inv_temp > 0 samples, tops the beam partials,
// hist the history rules, Wq the int8 table.
struct LogitsArgs {
  const _Float16* A = nullptr; int lda = 0;   // [B][K] fp16 rows
  const _Float16* W = nullptr;                // [V][K] fp16 table (null with Wq)
  // Wq / wscale (nullable; greedy, sampling and the history rules, no beam partials, no lnx): the
  // int8 table [V][K] and its row scales replace W: logit = wscale[v] * sum_k A[k] * fp16(Wq[v][k])
  const int8_t* Wq = nullptr; const float* wscale = nullptr;
  int K = 0, V = 0, B = 0;
  DecodeRules R{};
  const uint8_t* smask = nullptr;             // [V] suppressed tokens
  const RowRules* rules = nullptr;            // [B]
  LogitPart* parts = nullptr;                 // [B][nblk]
  // lnx: A = LayerNorm(lnx) (fp32 [B][K], eps 1e-5) computed in-block instead of read
  const float* lnx = nullptr; int ldx = 0; const float* ln_g = nullptr; const float* ln_b = nullptr;
  int max_blocks = 256;
  // R.inv_temp > 0: seeds [B] (device) per-row noise seeds, pos = the position whose logits
  // these are (the sampled token goes to pos + 1); row_inv_temp [B] (device, nullable): row
  // b samples at 1 / row_inv_temp[b] instead of R.inv_temp (several temperatures in one call)
  const uint32_t* seeds = nullptr; int pos = 0; const float* row_inv_temp = nullptr;
  // tops (nullable, greedy only; [B][nblk]): the beam instantiation — each partial also
  // carries its block's best kBeamTop allowed entries (BeamTop)
  BeamTop* tops = nullptr;
  // hist (nullable; greedy and sampling, no beam partials): the rows' history words
  // (history_rules_launch) — a penalised column's logit is scaled by rep_pen (> 0) before the
  // filter, a banned column fails it; the raw statistics stay unpenalised
  const uint32_t* hist = nullptr; float rep_pen = 1.f;
};
void logits_partial_launch(const LogitsArgs& a, hipStream_t s);
// The history words: uint32 [groups of logits_row_group(K) rows][(V + 15) / 16 tiles][rows of
// the group], bits 0-15 penalised / 16-31 banned columns of the tile. history_words: their
// count for B rows (zeroed by the caller before a call's first position).
size_t history_words(int V, int K, int B);
// one position's update for every row (one block per row, in front of logits_partial_launch
// at the same pos): tokens [B][ld], plen [B] prompt lengths, n = no_repeat_ngram_size
void history_rules_launch(const int32_t* tokens, int ld, int pos, const int32_t* plen, int n, int V,
                          int rg, uint32_t* hist, int B, hipStream_t s);
// What the selectors (select_partials_launch, select_embed_launch, beam_step_launch) share: a
// position's partials, the rules and the rows' state.
struct SelectArgs {
  const LogitPart* parts = nullptr; int nblk = 0;   // [rows][nblk]
  DecodeRules R{};
  RowRules* rules = nullptr;                        // [rows], rewritten for the next step
  int32_t* tokens = nullptr; int ld = 0;            // [rows][ld]
  int pos = 0;                                      // the selected token goes to pos + 1
  int32_t* done = nullptr; float* sum_lp = nullptr; int32_t* n_tok = nullptr;   // [rows]
  // plen [B] (device, nullable = all rows sample from pos + 1 >= 1): rows with pos + 1 <
  // plen[b] are still inside their own prompt and keep the forced token. At the step with
  // pos + 1 + R.target_back == plen[b] (target_back 0: the row's first sampled step; > 0: a
  // prompt position, where nothing else is touched) nsp[b] (nullable) gets the raw softmax
  // probability of DecodeRules::target (Whisper's no_speech_prob).
  const int32_t* plen = nullptr; float* nsp = nullptr;
  // per-row position offsets (staggered rows; embed_launch above). Not the beam step.
  const int32_t* roff = nullptr;
};
void select_partials_launch(const SelectArgs& a, int B, hipStream_t s);
// select_partials_launch at pos followed by embed_launch at pos + 1, in one launch
void select_embed_launch(const SelectArgs& a, int B, hipStream_t s, const _Float16* tok_emb,
                         const float* pos_emb, int d, float* x, float2* part, const float* ln_g,
                         const float* ln_b, _Float16* ln_out);
void build_mask_launch(const int32_t* list, int n, uint8_t* mask, int V, hipStream_t s);
// out [B][V] = sample_gumbel(noise_base(seeds[b], pos), t)
void sample_gumbel_launch(const uint32_t* seeds, int B, int pos, int V, float* out, hipStream_t s);

// ------------------------------------------------------------------ beam search (beam.hip)
// Device state of a beam decode: rows are windows x k (row w * k + j = beam j of window w).
struct BeamState {
  int k;                    // beam size, 1 .. kBeamMax
  float length_penalty;
  int32_t* nlive;           // [W] live beams (1 before a window's first sampled step)
  int32_t* nfin;            // [W] finished hypotheses
  int32_t* wdone;           // [W] the window stopped
  int32_t* moved;           // [W] the last step's parents are not the identity
  int32_t* parent;          // [W * k] parent beam (0 .. k-1) of each row after the last step
  int32_t* fin_tok;         // [W][k][ld] finished hypotheses: prompt, sampled tokens incl. eot
  float* fin_s;             // [W][k] their cumulative scores
  int32_t* fin_n;           // [W][k] their sampled tokens incl. eot
};
void beam_init_launch(const BeamState& st, int W, hipStream_t s);
// One block per window: the window's rows' partials -> the best 2k candidates (score
// descending, then beam, then token), the walk (eot candidates finish, the others become the
// next live beams), the children's tokens / scores / rule states, the finished list and
// the done flags. Rows inside their prompt keep the forced token with identity parents.
void beam_step_launch(const SelectArgs& a, const BeamTop* tops, const BeamState& st, int W, hipStream_t s);
// The self-attention caches follow the parents: row i of a window takes positions 0 .. pos
// of row parent[i], in place (a block loads its slab of every row of the window, then
// stores). kc / vc: [layers][W * k][n_ctx][d] fp16.
void beam_reorder_launch(_Float16* kc, _Float16* vc, int layers, int W, int k, int n_ctx, int d,
                         int pos, const int32_t* parent, const int32_t* moved, hipStream_t s);
// The winner of every window (finished hypothesis with the best S / n^length_penalty, the
// earliest on ties; none finished: the best live beam closed at n + 1) -> the call's outputs
void beam_finish_launch(const BeamState& st, const DecodeRules& R, const int32_t* tokens, int ld,
                        const float* sum_lp, const int32_t* n_tok, const int32_t* plen,
                        const float* nsp, int W, int32_t* tokens_out, int32_t* n_tokens_out,
                        float* sum_lp_out, float* nsp_out, hipStream_t s);
// kernel test: per row the best n2k entries of both sets merged over the row's nblk partials
// -> out_*[B][n2k] (unused: -inf / -1)
void beam_rowtop_launch(const BeamTop* tops, int nblk, int B, int n2k, float* all_v, int32_t* all_i,
                        float* ts_v, int32_t* ts_i, hipStream_t s);

}  // namespace janus

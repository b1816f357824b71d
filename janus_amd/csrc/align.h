// Word alignment kernels (align.hip) and the per-context state of janus_whisper_align.
#pragma once
#include "align_plan.h"
#include "common.h"
#include "devmem.h"

namespace janus {

// Token-tile attention: one block = 16 query rows of one (window, head); QK^T and PV on the
// fp16 MFMA, a full-row fp32 softmax in LDS. Serves the teacher-forced decoder's causal
// self-attention (Tk == 0: the window's own rows are the keys) and its cross-attention
// over Tk encoder frames (keys of window w at rows enc_row * Tk of k / v).
struct AlignAttnArgs {
  const _Float16* q; int64_t ldq;                        // packed row r, head h: q + r * ldq + 64 h
  const _Float16* k; const _Float16* v; int64_t ldkv;    // key row t: k + t * ldkv + 64 h
  _Float16* out; int64_t ldo;                            // packed rows [M][ldo]
  const AlignWinDev* wins; const int32_t* tiles;         // device tables (AlignPlan)
  int Tk; float scale;
  // alignment heads: head h writes its probabilities of frames < F, fp32, to slot
  // slots[h] of the window's [n_slots][n][F] block of probs (slots[h] < 0: no output)
  float* probs; int n_slots; int8_t slots[32];
};
void align_attention_launch(const AlignAttnArgs& a, int n_tiles, int H, int max_keys, hipStream_t s);

// x[r][:] = float(tok_emb[tok[r]]) + pos_emb[pos[r]] for M packed rows
void align_embed_launch(const _Float16* tok_emb, const float* pos_emb, const int32_t* tok,
                        const int32_t* pos, int M, int d, float* x, hipStream_t s);

// probs [heads][n][F] per window -> A [N][F]: (P - mean) / std over the n rows per (head,
// frame) (population std, fp64 accumulation), median of 7 along the frames with reflect
// padding (F <= 3: none), mean over heads, rows sot_len .. n - 2. stats: scratch, 2 doubles
// per (head, frame).
void align_reduce_launch(const float* probs, const AlignWinDev* wins, int n_windows, int heads,
                         int sot_len, int max_n, int max_F, double* stats, float* A, hipStream_t s);

// DTW over x = (negate ? -A : A) [N][F] of every window, one block each: anti-diagonal
// wavefront, three rolling diagonals in LDS, trace bytes [N + 1][F + 1] in global memory,
// backtrace on one lane. text_idx / time_idx [n_windows][path_stride] (-1 past the path),
// path_len [n_windows]; rev: scratch int32 [n_windows][2][path_stride]. N <= 511.
void align_dtw_launch(const float* A, const AlignWinDev* wins, int n_windows, int negate,
                      uint8_t* trace, int32_t* rev, int32_t* text_idx, int32_t* time_idx,
                      int32_t* path_len, int path_stride, hipStream_t s);

// Per row of logits [rows][ld] (fp32, V columns): out[out_idx[r]] = softmax(logits[r])[target[r]]
// (rows with out_idx < 0 are skipped).
void align_rowprob_launch(const float* logits, int64_t ld, int V, const int32_t* target,
                          const int32_t* out_idx, int rows, float* out, hipStream_t s);

// What a context keeps between janus_whisper_align calls: the alignment heads, the last
// call's plan (its host tables back the asynchronous uploads) and the workspaces.
struct AlignState {
  std::vector<int32_t> heads;  // (layer, head) pairs; empty: the default set
  AlignPlan plan;
  DevMem d_x, d_a, d_qkv, d_o, d_q2, d_f, d_ck, d_cv, d_probs, d_stats, d_A, d_trace, d_rev,
      d_logits, d_wins, d_tiles, d_tok, d_pos, d_target, d_oidx;
};

}  // namespace janus

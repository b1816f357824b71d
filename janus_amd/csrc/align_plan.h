// Word alignment (janus_whisper_align): the host-side plan of one call — validation of the
// caller's arrays and the packed-row / tile / buffer layout the kernels of align.hip index.
// Free of HIP headers, like decode_plan.h: a stand-alone host program can drive it.
#pragma once

#include <cstdint>
#include <vector>
#include "errors.h"

namespace janus {

constexpr int kAlignMaxHeads = 64;    // alignment heads of one context
constexpr int kAlignMedian = 7;       // median filter width along the frames
constexpr int kAlignTileRows = 16;    // query rows of one attention block (one MFMA m-tile)
constexpr int kAlignMaxSizeFrames = 3000;

// One window as the kernels see it (device table, one entry per window).
struct AlignWinDev {
  int32_t row0;     // first of the window's n packed rows
  int32_t n;        // sequence length: sot_len + 1 + len(text) + 1
  int32_t enc_row;  // encoder row the window attends to
  int32_t F;        // frames kept: size / 2
  int32_t N;        // rows of A: len(text) + 1
  int32_t pad;
  int64_t poff;     // floats: the window's probabilities [heads][n][F]
  int64_t soff;     // entries: its per (head, frame) mean / std [heads][F]
  int64_t aoff;     // floats: its A [N][F] (windows packed back to back)
  int64_t toff;     // bytes: its DTW trace [N + 1][F + 1]
};

struct AlignPlan {
  int n_windows = 0, M = 0, sot_len = 0, eot = 0, heads = 0, max_n = 0;
  std::vector<AlignWinDev> wins;
  std::vector<int32_t> tiles;    // (window, first query row) per attention block
  std::vector<int32_t> tok, pos;  // per packed row: token id, position
  std::vector<int32_t> target;   // per packed row: the forced next token (-1: none)
  std::vector<int32_t> out_idx;  // per packed row: index into token_probs (-1: none)
  int64_t probs_total = 0, stats_total = 0, a_total = 0, trace_total = 0;
  int n_tiles() const { return (int)(tiles.size() / 2); }
};

// Validates (layer, head) pairs against the model: 1 .. kAlignMaxHeads pairs, indices in
// range, no pair twice. Throws janus::Error.
void align_check_heads(int dec_layers, int n_heads, const int32_t* pairs, int n_pairs);
// The default: every head of the last half of the decoder layers (l >= dec_layers / 2), or
// throws when those are more than kAlignMaxHeads.
std::vector<int32_t> align_default_heads(int dec_layers, int n_heads);

// tokens [n_windows][stride] (window w's seq in its first token_lens[w] entries), sizes in mel
// frames, enc_index nullable (window w attends to encoder row w; then n_enc >= n_windows).
// Throws janus::Error on any argument the call must reject.
AlignPlan align_plan(int n_text_ctx, int n_vocab, int heads, int n_enc, int n_windows,
                     const int32_t* tokens, const int32_t* token_lens, int stride,
                     const int32_t* sizes, const int32_t* enc_index, int sot_len, int eot,
                     int path_stride);

}  // namespace janus

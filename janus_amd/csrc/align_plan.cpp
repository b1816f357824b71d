// The host-side plan of a janus_whisper_align call (align_plan.h): validation and layout.
#include "align_plan.h"

#include <set>
#include <string>
#include <utility>

namespace janus {

void align_check_heads(int dec_layers, int n_heads, const int32_t* pairs, int n_pairs) {
  JANUS_CHECK(pairs && n_pairs >= 1, "alignment heads: at least one (layer, head) pair");
  JANUS_CHECK(n_pairs <= kAlignMaxHeads,
              "alignment heads: at most " + std::to_string(kAlignMaxHeads) + " pairs");
  std::set<std::pair<int, int>> seen;
  for (int i = 0; i < n_pairs; ++i) {
    const int l = pairs[2 * i], h = pairs[2 * i + 1];
    JANUS_CHECK(l >= 0 && l < dec_layers && h >= 0 && h < n_heads,
                "alignment heads: (" + std::to_string(l) + ", " + std::to_string(h) + ") out of range");
    JANUS_CHECK(seen.insert({l, h}).second, "alignment heads: a pair is listed twice");
  }
}

std::vector<int32_t> align_default_heads(int dec_layers, int n_heads) {
  std::vector<int32_t> out;
  for (int l = dec_layers / 2; l < dec_layers; ++l)
    for (int h = 0; h < n_heads; ++h) {
      out.push_back(l);
      out.push_back(h);
    }
  JANUS_CHECK(!out.empty() && (int)out.size() / 2 <= kAlignMaxHeads,
              "alignment heads: the default set exceeds " + std::to_string(kAlignMaxHeads) +
                  " heads; name them (janus_whisper_set_alignment_heads)");
  return out;
}

AlignPlan align_plan(int n_text_ctx, int n_vocab, int heads, int n_enc, int n_windows,
                     const int32_t* tokens, const int32_t* token_lens, int stride,
                     const int32_t* sizes, const int32_t* enc_index, int sot_len, int eot,
                     int path_stride) {
  JANUS_CHECK(tokens && token_lens && sizes, "align: null argument");
  JANUS_CHECK(n_windows >= 1 && n_windows <= 4096, "align: 1 .. 4096 windows");
  JANUS_CHECK(heads >= 1 && heads <= kAlignMaxHeads, "align: no alignment heads");
  JANUS_CHECK(sot_len >= 1 && eot >= 1 && eot < n_vocab, "align: bad sot_len / eot");
  JANUS_CHECK(stride >= 1 && path_stride >= 1, "align: bad stride");
  JANUS_CHECK(n_enc >= 1 && (enc_index || n_enc >= n_windows), "align: fewer encoder rows than windows");
  AlignPlan P;
  P.n_windows = n_windows; P.sot_len = sot_len; P.eot = eot; P.heads = heads;
  P.wins.resize(n_windows);
  int64_t rows = 0;
  for (int w = 0; w < n_windows; ++w) {
    const int n = token_lens[w], size = sizes[w];
    const std::string at = " (window " + std::to_string(w) + ")";
    // sot_sequence + <|notimestamps|> + at least one text token + eot
    JANUS_CHECK(n >= sot_len + 3, "align: a window needs at least one text token" + at);
    JANUS_CHECK(n <= n_text_ctx, "align: sequence longer than n_text_ctx" + at);
    JANUS_CHECK(n <= stride, "align: token_lens exceeds the token stride" + at);
    JANUS_CHECK(size >= 2 && size <= kAlignMaxSizeFrames, "align: size must lie in [2, 3000]" + at);
    const int32_t* seq = tokens + (int64_t)w * stride;
    for (int i = 0; i < n; ++i)
      JANUS_CHECK(seq[i] >= 0 && seq[i] < n_vocab, "align: token id out of range" + at);
    for (int i = sot_len + 1; i < n - 1; ++i)
      JANUS_CHECK(seq[i] < eot, "align: text tokens must be < eot" + at);
    JANUS_CHECK(seq[n - 1] == eot, "align: the sequence must end in eot" + at);
    const int e = enc_index ? enc_index[w] : w;
    JANUS_CHECK(e >= 0 && e < n_enc, "align: enc_index out of range" + at);
    AlignWinDev& W = P.wins[w];
    W.row0 = (int32_t)rows; W.n = n; W.enc_row = e; W.F = size / 2; W.N = n - sot_len - 1; W.pad = 0;
    JANUS_CHECK(W.N + W.F <= path_stride, "align: path_stride below N + F" + at);
    W.poff = P.probs_total; W.soff = P.stats_total; W.aoff = P.a_total; W.toff = P.trace_total;
    P.probs_total += (int64_t)heads * n * W.F;
    P.stats_total += (int64_t)heads * W.F;
    P.a_total += (int64_t)W.N * W.F;
    P.trace_total += (int64_t)(W.N + 1) * (W.F + 1);
    for (int q0 = 0; q0 < n; q0 += kAlignTileRows) {
      P.tiles.push_back(w);
      P.tiles.push_back(q0);
    }
    for (int i = 0; i < n; ++i) {
      P.tok.push_back(seq[i]);
      P.pos.push_back(i);
      // row sot_len + r predicts text[r] = seq[sot_len + 1 + r], r < len(text) = N - 1
      const int r = i - sot_len;
      const bool forced = r >= 0 && r < W.N - 1;
      P.target.push_back(forced ? seq[i + 1] : -1);
      P.out_idx.push_back(forced ? w * stride + r : -1);
    }
    rows += n;
    if (n > P.max_n) P.max_n = n;
  }
  JANUS_CHECK(rows < (1ll << 30), "align: too many rows");
  P.M = (int)rows;
  return P;
}

}  // namespace janus

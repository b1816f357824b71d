// What the decode planner (decode_plan.cpp) shares with the kernels' headers, free of HIP
// headers: the row limits, the decoding rules and the pure shape predicates. kernels.h and
// decoder.h include this file for the constants and DecodeRules; the predicates are declared
// again here exactly as beside their launchers (kernels.h, decoder.h, dec_persist.h), where
// their comments live.
#pragma once

namespace janus {

// Largest M the skinny (decoder-step) GEMM takes: a decode batch of 64 windows x 5 sampled
// hypotheses (faster-whisper's best_of) is 320 rows.
constexpr int kSkinnyMaxRows = 512;
constexpr int kBeamMax = 8;

struct DecodeRules {
  int eot;
  int suppress_blank, blank;     // SuppressBlank at the first sampled token
  int ts_begin;                  // first timestamp token id; -1 disables timestamp rules
  int no_timestamps;             // <|notimestamps|> (always suppressed in timestamp mode)
  int max_initial_ts;            // max_initial_timestamp index (-1: none)
  int target;                    // token whose raw softmax probability is tracked (no-speech), -1: none
  float inv_temp;                // 0: greedy (argmax); > 0: sample at temperature 1 / inv_temp
                                 // (Gumbel-max over the rule-filtered logits, noise from
                                 // sample_noise(seed of the row, position, token))
  int target_back = 0;           // target's probability is read target_back positions before the
                                 // row's last prompt position (janus_decode_rows.no_speech_back)
};

bool resid_ln_supported(int N, int K);
bool xattn_supported(int D, int H);
int xattn_split_count(int Te, int requested);
bool xattn_rows_supported(int D, int H);
int xattn_rows_max(int D, int H);
bool xattn_cvp_supported(int D, int H);
int logits_partial_blocks(int V, int K, int max_blocks);
bool dec_seg_supported(int d, int H, int B, int cus);

}  // namespace janus

// The Whisper context as whisper.cpp (weights, log-mel, encoder) and decode.cpp (the decode
// call) share it: the prepared layers, the decoder lanes and struct janus_whisper.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "align.h"
#include "devmem.h"
#include "kernels.h"
#include "../../include/janus.h"

namespace janus {

struct EncLayer {
  DevMem wqkv, bqkv, wo, w1, w2;  // fp16 weights / fp32 fused bias
  // int8 copies of the same four weights, quantised per output row from the fp32 parameters,
  // and their dequantisation scales (prepare_i8: made when the int8 encoder is first used)
  DevMem qqkv, sqkv, qo, so, q1, s1, q2, s2;
  const float *bo, *b1, *b2, *ln1g, *ln1b, *ln2g, *ln2b;
};
struct DecLayer {
  DevMem wqkv, bqkv, wo, wq_c, wk_c, wv_c, wo_c, w1, w2;
  DevMem wqk, bqk;  // absorbed cross-attention query weights (xattn.hip)
  // int8 copies of the seven matrices the decode call multiplies and their row scales,
  // quantised from the fp16 copies above (prepare_dec_i8: made when the int8 decoder weights
  // are first used), indexed by JANUS_DEC_W_*
  DevMem q8[7], s8[7];
  const DevMem& w16(int which) const {
    const DevMem* m[7] = {&wqkv, &wo, &wqk, &wv_c, &wo_c, &w1, &w2};
    return *m[which];
  }
  const float *bo, *bq_c, *bv_c, *bo_c, *b1, *b2;
  const float *ln1g, *ln1b, *ln2g, *ln2b, *ln3g, *ln3b;
};

// One decoder lane: the per-step workspaces, KV caches and captured decode graphs for one
// slice of the batch, plus the stream it runs on. Independent lanes run concurrently
// (one host thread and one HIP stream each): every decoder launch is latency-bound at
// B <= 64, so two half-batch chains overlap their launch and memory round trips.
struct DecLane {
  DevMem d_x, d_a, d_qkv, d_o, d_q2, d_f, d_kc, d_vc, d_ck, d_cv, d_smask, d_done, d_prompt, d_nsp,
      d_supp, d_part_o, d_part_ml, d_parts, d_rules, d_tok, d_ntok, d_slp, d_lnp, d_lncnt, d_xqk,
      d_xc, d_xpc, d_xpml, d_enc, d_seed, d_xpairs, d_xgroups, d_roff, d_omid, d_segbar, d_segerr,
      d_itemp, d_btop, d_bint, d_bfin, d_bfs,   // (beam search: partial tops, window state, finished list)
      d_hist,                                   // (history rules: the rows' penalised / banned bit sets)
      // int8 cross-attention: the rows' quantised encoder output and per-key scales as the
      // kernels read them, and the shared rows' before the gather (gathered rows only)
      d_encq, d_encs, d_encq0, d_encs0;
  std::map<std::vector<int64_t>, hipGraphExec_t> graphs;
  std::map<std::vector<int64_t>, size_t> graph_nodes;  // kernel nodes per captured graph
  // the path the last decode call took (janus_whisper_decode_path): how its rows reached
  // their encoder output (JANUS_ENC_ROWS_*) and the persistent level it ran (0: launches)
  int last_enc_rows = 0, last_persist = 0;
  int last_cross = 0;            // JANUS_CROSS_COMPUTE_* the last call ran (janus_whisper_decode_cross)
  int last_weights = 0;          // JANUS_DEC_COMPUTE_* the last call ran (janus_whisper_decode_weights)
  int last_positions = 0;        // positions the last decode stepped
  int64_t last_launches = 0;     // kernel launches those positions issued (graph nodes)
  // where each row slot stands after the last call (positions whose KV rows and next
  // tokens are written): a staggered call may continue row b only from an offset <=
  // stand[b], with the same batch size and max_length. Empty: nothing to continue (no call
  // yet, or the last one failed).
  std::vector<int32_t> stand;
  int stand_maxlen = 0;
  hipStream_t stream = nullptr;  // graph capture needs a non-null stream
  std::vector<uint32_t> stream_mask;  // CU mask the lane stream was created with (empty: none)
  hipEvent_t ev_done = nullptr;
  // a call without early-exit polling (check_every 0) returns without waiting for its
  // stream: its persistent segments' barrier-timeout flag is copied to pinned h_segerr
  // behind it and checked by janus_whisper_decode_check (or at this lane's next call)
  uint32_t* h_segerr = nullptr;
  hipEvent_t ev_segerr = nullptr;
  bool segerr_pending = false;
  DecLane() = default;
  DecLane(const DecLane&) = delete;
  DecLane& operator=(const DecLane&) = delete;
  void drop_graphs() {
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
    graph_nodes.clear();
  }
  ~DecLane() {
    drop_graphs();
    if (stream) (void)hipStreamDestroy(stream);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (ev_segerr) (void)hipEventDestroy(ev_segerr);
    if (h_segerr) (void)hipHostFree(h_segerr);
  }
};

}  // namespace janus

struct janus_whisper {
  janus_whisper_config cfg;
  janus::ParamStore params;
  bool prepared = false;
  int enc_compute = JANUS_ENC_COMPUTE_F16;  // janus_whisper_set_encoder_compute
  bool i8_prepared = false;                 // the encoder layers hold their int8 weights
  int cross_compute = JANUS_CROSS_COMPUTE_F16;  // janus_whisper_set_cross_compute
  int dec_compute = JANUS_DEC_COMPUTE_F16;      // janus_whisper_set_decoder_compute
  bool dec_i8_prepared = false;                 // the decoder layers and tokq hold their int8 weights
  std::mutex mu;
  // device-side prepared weights
  janus::DevMem conv1p, conv2p, pos16, tok16;
  janus::DevMem tokq, toks;  // int8 decoder weights: the vocabulary projection's table and row scales
  std::vector<janus::EncLayer> enc;
  std::vector<janus::DecLayer> dec;
  // workspaces
  janus::DevMem ws_x1, ws_x2, ws_r, ws_a, ws_qkv, ws_o, ws_f, ws_logmel, ws_maxkey;
  janus::DevMem ws_q8, ws_qs;  // int8 encoder: quantised GEMM input rows and their scales
  // decoder lanes: each owns the workspaces, captured graphs and stream of one batch slice
  std::vector<std::unique_ptr<janus::DecLane>> lanes;
  int last_slot = 0;  // state slot of the last decode call (decode_info reports it)
  // language identification's own lane (janus_whisper_detect_language): no state slot's KV
  // cache, tokens, graphs or stand is touched by it
  std::unique_ptr<janus::DecLane> lang_lane;
  janus::AlignState align;  // word alignment (align_call.cpp): heads, plan and workspaces
  hipEvent_t ev_in = nullptr;
  ~janus_whisper() {
    if (ev_in) (void)hipEventDestroy(ev_in);
  }
};

namespace janus {

// the device-side weights from the uploaded parameters (whisper.cpp; no-op once prepared)
void prepare(janus_whisper* w, hipStream_t s);
// the int8 copies of the decoder's weights (whisper.cpp; after prepare, no-op once made)
void prepare_dec_i8(janus_whisper* w, hipStream_t s);
// rows and columns of a decoder layer's matrix JANUS_DEC_W_* (which), or of the vocabulary table (-1)
inline void dec_weight_shape(const janus_whisper_config& c, int which, int64_t* N, int64_t* K) {
  const int64_t d = c.d_model;
  *K = which == JANUS_DEC_W_FC2 ? 4 * d : d;
  *N = which < 0 ? c.n_vocab : which == JANUS_DEC_W_QKV ? 3 * d : which == JANUS_DEC_W_XQK ? c.n_heads * d
       : which == JANUS_DEC_W_FC1 ? 4 * d : d;
}

inline GemmArgs gargs(const _Float16* A, int64_t lda, const _Float16* W, int64_t ldw,
                      const float* bias, void* C, int64_t ldc, int M, int N, int K,
                      const float* R = nullptr, int64_t ldr = 0) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc;
  g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
  return g;
}

}  // namespace janus

// janus_whisper_align (include/janus.h): the alignment pass of word-level timestamps. One
// call aligns several windows of different lengths: their token sequences are packed row
// after row, the decoder runs over all rows teacher-forced (the linear layers on the GEMM /
// LayerNorm launchers, attention on align.hip's token-tile kernel), the alignment heads'
// cross-attention probabilities are reduced to one matrix per window and a DTW solve per
// window gives the path. No decoder state slot is touched: a call between two staggered
// decode calls leaves them as they were.
#include <algorithm>
#include "decoder.h"
#include "whisper_internal.h"

namespace janus {

namespace {

constexpr int kLogitRows = 256;  // rows of one vocabulary-projection chunk ([rows][eot] fp32)

template <class T>
const T* upload(DevMem& m, const std::vector<T>& v, hipStream_t s) {
  m.ensure(sizeof(T) * std::max<size_t>(v.size(), 1));
  if (!v.empty())
    JANUS_HIP(hipMemcpyAsync(m.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s));
  return m.as<T>();
}

}  // namespace

static void align_run(janus_whisper* w, const _Float16* enc, int n_enc, int n_windows,
                      const int32_t* tokens, const int32_t* token_lens, int stride,
                      const int32_t* sizes, const int32_t* enc_index, int sot_len, int eot,
                      int32_t* text_idx, int32_t* time_idx, int32_t* path_len, int path_stride,
                      float* token_probs, float* attn_out, int phases, hipStream_t s) {
  const auto& c = w->cfg;
  const int d = c.d_model, H = c.n_heads, Te = c.n_audio_ctx, ff = 4 * d;
  AlignState& Z = w->align;
  if (Z.heads.empty()) Z.heads = align_default_heads(c.dec_layers, H);
  const int heads = (int)Z.heads.size() / 2;
  JANUS_CHECK(H <= 32, "align: at most 32 heads per layer");
  JANUS_CHECK(d <= 1024, "align: d_model <= 1024 (the alignment pass is not built for the 1280-wide models)");
  JANUS_CHECK((int64_t)n_enc * Te < (1ll << 31), "align: too many encoder rows");
  // the previous call's plan backs its uploads: let them finish before it is replaced
  JANUS_HIP(hipStreamSynchronize(s));
  Z.plan = align_plan(c.n_text_ctx, c.n_vocab, heads, n_enc, n_windows, tokens, token_lens, stride,
                      sizes, enc_index, sot_len, eot, path_stride);
  const AlignPlan& P = Z.plan;
  JANUS_CHECK(P.max_n - sot_len - 1 <= 511, "align: at most 511 aligned rows per window");
  const int M = P.M;
  if (phases == 0) phases = 7;
  prepare(w, s);

  const AlignWinDev* wins = upload(Z.d_wins, P.wins, s);
  const int32_t* tiles = upload(Z.d_tiles, P.tiles, s);
  const int32_t* tok = upload(Z.d_tok, P.tok, s);
  const int32_t* pos = upload(Z.d_pos, P.pos, s);
  const int32_t* target = upload(Z.d_target, P.target, s);
  const int32_t* oidx = upload(Z.d_oidx, P.out_idx, s);
  const int vpad = (eot + 7) & ~7;
  Z.d_x.ensure(sizeof(float) * (size_t)M * d);
  Z.d_a.ensure(sizeof(_Float16) * (size_t)M * d);
  Z.d_qkv.ensure(sizeof(_Float16) * (size_t)M * 3 * d);
  Z.d_o.ensure(sizeof(_Float16) * (size_t)M * d);
  Z.d_q2.ensure(sizeof(_Float16) * (size_t)M * d);
  Z.d_f.ensure(sizeof(_Float16) * (size_t)M * ff);
  Z.d_ck.ensure(sizeof(_Float16) * (size_t)n_enc * Te * d);
  Z.d_cv.ensure(sizeof(_Float16) * (size_t)n_enc * Te * d);
  Z.d_probs.ensure(sizeof(float) * (size_t)P.probs_total);
  Z.d_stats.ensure(sizeof(double) * 2 * (size_t)P.stats_total);
  Z.d_A.ensure(sizeof(float) * (size_t)P.a_total);
  Z.d_trace.ensure((size_t)P.trace_total);
  Z.d_rev.ensure(sizeof(int32_t) * (size_t)n_windows * 2 * path_stride);
  Z.d_logits.ensure(sizeof(float) * (size_t)std::min(M, kLogitRows) * vpad);
  float* x = Z.d_x.as<float>();
  _Float16 *a = Z.d_a.as<_Float16>(), *qkv = Z.d_qkv.as<_Float16>(), *o = Z.d_o.as<_Float16>(),
           *q2 = Z.d_q2.as<_Float16>(), *f = Z.d_f.as<_Float16>(), *ck = Z.d_ck.as<_Float16>(),
           *cv = Z.d_cv.as<_Float16>();
  float* probs = Z.d_probs.as<float>();
  float* A = Z.d_A.as<float>();

  if (phases & 1) {
    align_embed_launch(w->tok16.as<_Float16>(),
                       w->params.get("decoder.embed_positions.weight", (int64_t)c.n_text_ctx * d),
                       tok, pos, M, d, x, s);
    const int ME = n_enc * Te;
    for (int l = 0; l < c.dec_layers; ++l) {
      DecLayer& L = w->dec[l];
      layernorm_launch(x, L.ln1g, L.ln1b, a, M, d, 1e-5f, s);
      gemm_launch(EPI_F16, gargs(a, d, L.wqkv.as<_Float16>(), d, L.bqkv.as<float>(), qkv, 3 * d, M, 3 * d, d), s);
      AlignAttnArgs at{};
      at.q = qkv; at.ldq = 3 * d; at.k = qkv + d; at.v = qkv + 2 * d; at.ldkv = 3 * d;
      at.out = o; at.ldo = d; at.wins = wins; at.tiles = tiles; at.Tk = 0; at.scale = 0.125f;
      at.probs = nullptr; at.n_slots = 0;
      for (int h = 0; h < 32; ++h) at.slots[h] = -1;
      align_attention_launch(at, P.n_tiles(), H, P.max_n, s);
      gemm_launch(EPI_RESID_F32, gargs(o, d, L.wo.as<_Float16>(), d, L.bo, x, d, M, d, d, x, d), s);
      layernorm_launch(x, L.ln2g, L.ln2b, a, M, d, 1e-5f, s);
      gemm_launch(EPI_F16, gargs(a, d, L.wq_c.as<_Float16>(), d, L.bq_c, q2, d, M, d, d), s);
      // the plain cross K / V projections of the encoder rows (k_proj has no bias)
      gemm_launch(EPI_F16, gargs(enc, d, L.wk_c.as<_Float16>(), d, nullptr, ck, d, ME, d, d), s);
      gemm_launch(EPI_F16, gargs(enc, d, L.wv_c.as<_Float16>(), d, L.bv_c, cv, d, ME, d, d), s);
      AlignAttnArgs ax = at;
      ax.q = q2; ax.ldq = d; ax.k = ck; ax.v = cv; ax.ldkv = d; ax.Tk = Te;
      bool any = false;
      for (int i = 0; i < heads; ++i)
        if (Z.heads[2 * i] == l) {
          ax.slots[Z.heads[2 * i + 1]] = (int8_t)i;
          any = true;
        }
      ax.probs = any ? probs : nullptr;
      ax.n_slots = heads;
      align_attention_launch(ax, P.n_tiles(), H, Te, s);
      gemm_launch(EPI_RESID_F32, gargs(o, d, L.wo_c.as<_Float16>(), d, L.bo_c, x, d, M, d, d, x, d), s);
      layernorm_launch(x, L.ln3g, L.ln3b, a, M, d, 1e-5f, s);
      gemm_launch(EPI_GELU_F16, gargs(a, d, L.w1.as<_Float16>(), d, L.b1, f, ff, M, ff, d), s);
      gemm_launch(EPI_RESID_F32, gargs(f, ff, L.w2.as<_Float16>(), ff, L.b2, x, d, M, d, ff, x, d), s);
    }
    layernorm_launch(x, w->params.get("decoder.layer_norm.weight", d),
                     w->params.get("decoder.layer_norm.bias", d), a, M, d, 1e-5f, s);
    // forced-token probabilities: logits over ids < eot, one chunk of rows at a time
    JANUS_HIP(hipMemsetAsync(token_probs, 0, sizeof(float) * (size_t)n_windows * stride, s));
    float* logits = Z.d_logits.as<float>();
    for (int r0 = 0; r0 < M; r0 += kLogitRows) {
      const int rows = std::min(kLogitRows, M - r0);
      gemm_nt128_launch(EPI_F32, gargs(a + (int64_t)r0 * d, d, w->tok16.as<_Float16>(), d, nullptr, logits,
                                       vpad, rows, eot, d), s);
      align_rowprob_launch(logits, vpad, eot, target + r0, oidx + r0, rows, token_probs, s);
    }
  }
  int max_F = 0;
  for (const auto& W : P.wins) max_F = std::max(max_F, (int)W.F);
  if (phases & 2) {
    align_reduce_launch(probs, wins, n_windows, heads, sot_len, P.max_n, max_F, Z.d_stats.as<double>(), A, s);
    if (attn_out)
      JANUS_HIP(hipMemcpyAsync(attn_out, A, sizeof(float) * (size_t)P.a_total, hipMemcpyDeviceToDevice, s));
  }
  if (phases & 4)
    align_dtw_launch(A, wins, n_windows, 1, Z.d_trace.as<uint8_t>(), Z.d_rev.as<int32_t>(), text_idx,
                     time_idx, path_len, path_stride, s);
}

}  // namespace janus

using namespace janus;

extern "C" int janus_whisper_set_alignment_heads(janus_whisper* w, const int32_t* pairs, int n_pairs) {
  return guarded([&] {
    JANUS_CHECK(w, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    if (!pairs && n_pairs == 0) {   // back to the default set
      w->align.heads.clear();
      return;
    }
    align_check_heads(w->cfg.dec_layers, w->cfg.n_heads, pairs, n_pairs);
    w->align.heads.assign(pairs, pairs + 2 * (size_t)n_pairs);
  });
}

extern "C" int janus_whisper_align(janus_whisper* w, const uint16_t* enc, int n_enc, int n_windows,
                                   const int32_t* tokens, const int32_t* token_lens, int stride,
                                   const int32_t* sizes, const int32_t* enc_index, int sot_len, int eot,
                                   int32_t* text_indices, int32_t* time_indices, int32_t* path_lens,
                                   int path_stride, float* token_probs, float* attn_out, int phases,
                                   void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && enc && text_indices && time_indices && path_lens && token_probs, "null argument");
    JANUS_CHECK(phases >= 0 && phases <= 7, "align: phases is a mask of 1 (forward), 2 (reduce), 4 (DTW)");
    std::lock_guard<std::mutex> lk(w->mu);
    align_run(w, reinterpret_cast<const _Float16*>(enc), n_enc, n_windows, tokens, token_lens, stride,
              sizes, enc_index, sot_len, eot, text_indices, time_indices, path_lens, path_stride,
              token_probs, attn_out, phases, (hipStream_t)stream);
  });
}

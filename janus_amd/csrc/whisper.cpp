// Whisper STT on gfx950: log-mel -> encoder -> batched greedy decoder. This file: the
// weights, the log-mel front end and the encoder; the decode call is decode.cpp.
//
// Replaces faster-whisper's WhisperModel (CTranslate2, int8 on CPU) as driven by
// Transcriber.transcribe_buffer (backend/services/transcriber.py:29-64):
// model.transcribe(audio[::3], beam_size=1, language='en') for one 30 s window.
// Weights arrive by name (HF Whisper checkpoint naming) as fp32 and are re-laid out
// on the device: fused fp16 QKV, packed conv weights, fp16 embeddings; the residual
// stream stays fp32, GEMM/attention operands are fp16 on MFMA with fp32 accumulation.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "decoder.h"
#include "whisper_internal.h"

namespace janus {

static _Float16* to_f16(const float* src, int64_t n, DevMem& dst, hipStream_t s) {
  dst.ensure(sizeof(_Float16) * n);
  cast_f32_f16_launch(src, dst.as<_Float16>(), n, s);
  return dst.as<_Float16>();
}

// concat rows of fp32 matrices into one fp16 matrix (missing name => zeros)
static void fuse_f16(const ParamStore& P, const std::vector<std::string>& names, int64_t each,
                     DevMem& dst, hipStream_t s) {
  dst.ensure(sizeof(_Float16) * each * names.size());
  for (size_t i = 0; i < names.size(); ++i) {
    _Float16* d = dst.as<_Float16>() + i * each;
    if (P.has(names[i])) cast_f32_f16_launch(P.get(names[i], each), d, each, s);
    else JANUS_HIP(hipMemsetAsync(d, 0, sizeof(_Float16) * each, s));
  }
}

static void fuse_f32(const ParamStore& P, const std::vector<std::string>& names, int64_t each,
                     DevMem& dst, hipStream_t s) {
  dst.ensure(sizeof(float) * each * names.size());
  for (size_t i = 0; i < names.size(); ++i) {
    float* d = dst.as<float>() + i * each;
    if (P.has(names[i]))
      JANUS_HIP(hipMemcpyAsync(d, P.get(names[i], each), sizeof(float) * each,
                               hipMemcpyDeviceToDevice, s));
    else JANUS_HIP(hipMemsetAsync(d, 0, sizeof(float) * each, s));
  }
}

void prepare(janus_whisper* w, hipStream_t s) {
  if (w->prepared) return;
  // the captured decode graphs bake in the device weight pointers that are re-allocated
  // below: drop them (a set_tensor after a decode must not replay freed weights)
  JANUS_HIP(hipDeviceSynchronize());
  for (auto& lane : w->lanes) lane->drop_graphs();
  const auto& c = w->cfg;
  const int d = c.d_model, ff = 4 * d;
  const ParamStore& P = w->params;
  auto pk = [&](const std::string& name, int cin, DevMem& dst) {
    const float* src = P.get(name, (int64_t)d * cin * 3);
    const ConvPack g = conv_pack_geometry(cin, d, 3);
    dst.ensure(sizeof(_Float16) * g.phase_elems);
    conv_pack_weights(src, dst.as<_Float16>(), cin, d, 3, 0, 1, s);
  };
  pk("encoder.conv1.weight", c.n_mels, w->conv1p);
  pk("encoder.conv2.weight", d, w->conv2p);
  to_f16(P.get("encoder.embed_positions.weight", (int64_t)c.n_audio_ctx * d),
         (int64_t)c.n_audio_ctx * d, w->pos16, s);
  to_f16(P.get("decoder.embed_tokens.weight", (int64_t)c.n_vocab * d), (int64_t)c.n_vocab * d,
         w->tok16, s);
  const int64_t dd = (int64_t)d * d, fd = (int64_t)ff * d;
  w->enc.clear();
  w->enc.resize(c.enc_layers);
  w->i8_prepared = false;  // the int8 copies went with the layers
  for (int l = 0; l < c.enc_layers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    EncLayer& L = w->enc[l];
    fuse_f16(P, {p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"}, dd, L.wqkv, s);
    fuse_f32(P, {p + "self_attn.q_proj.bias", p + "self_attn.k_proj.bias", p + "self_attn.v_proj.bias"}, d, L.bqkv, s);
    to_f16(P.get(p + "self_attn.out_proj.weight", dd), dd, L.wo, s);
    to_f16(P.get(p + "fc1.weight", fd), fd, L.w1, s);
    to_f16(P.get(p + "fc2.weight", fd), fd, L.w2, s);
    L.bo = P.get(p + "self_attn.out_proj.bias", d);
    L.b1 = P.get(p + "fc1.bias", ff);
    L.b2 = P.get(p + "fc2.bias", d);
    L.ln1g = P.get(p + "self_attn_layer_norm.weight", d);
    L.ln1b = P.get(p + "self_attn_layer_norm.bias", d);
    L.ln2g = P.get(p + "final_layer_norm.weight", d);
    L.ln2b = P.get(p + "final_layer_norm.bias", d);
  }
  w->dec.clear();
  w->dec.resize(c.dec_layers);
  w->dec_i8_prepared = false;  // likewise the decoder's
  for (int l = 0; l < c.dec_layers; ++l) {
    const std::string p = "decoder.layers." + std::to_string(l) + ".";
    DecLayer& L = w->dec[l];
    fuse_f16(P, {p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"}, dd, L.wqkv, s);
    fuse_f32(P, {p + "self_attn.q_proj.bias", p + "self_attn.k_proj.bias", p + "self_attn.v_proj.bias"}, d, L.bqkv, s);
    to_f16(P.get(p + "self_attn.out_proj.weight", dd), dd, L.wo, s);
    to_f16(P.get(p + "encoder_attn.q_proj.weight", dd), dd, L.wq_c, s);
    to_f16(P.get(p + "encoder_attn.k_proj.weight", dd), dd, L.wk_c, s);
    to_f16(P.get(p + "encoder_attn.v_proj.weight", dd), dd, L.wv_c, s);
    to_f16(P.get(p + "encoder_attn.out_proj.weight", dd), dd, L.wo_c, s);
    to_f16(P.get(p + "fc1.weight", fd), fd, L.w1, s);
    to_f16(P.get(p + "fc2.weight", fd), fd, L.w2, s);
    L.bo = P.get(p + "self_attn.out_proj.bias", d);
    L.bq_c = P.get(p + "encoder_attn.q_proj.bias", d);
    L.bv_c = P.get(p + "encoder_attn.v_proj.bias", d);
    L.bo_c = P.get(p + "encoder_attn.out_proj.bias", d);
    L.b1 = P.get(p + "fc1.bias", ff);
    L.b2 = P.get(p + "fc2.bias", d);
    L.ln1g = P.get(p + "self_attn_layer_norm.weight", d);
    L.ln1b = P.get(p + "self_attn_layer_norm.bias", d);
    L.ln2g = P.get(p + "encoder_attn_layer_norm.weight", d);
    L.ln2b = P.get(p + "encoder_attn_layer_norm.bias", d);
    L.ln3g = P.get(p + "final_layer_norm.weight", d);
    L.ln3b = P.get(p + "final_layer_norm.bias", d);
    if (xattn_supported(d, c.n_heads)) {
      const int64_t hd = (int64_t)c.n_heads * d;
      L.wqk.ensure(sizeof(_Float16) * hd * d);
      L.bqk.ensure(sizeof(float) * hd);
      const std::string e = p + "encoder_attn.";
      xattn_absorb(P.get(e + "q_proj.weight", dd), P.has(e + "q_proj.bias") ? P.get(e + "q_proj.bias", d) : nullptr,
                   P.get(e + "k_proj.weight", dd), d, c.n_heads, L.wqk.as<_Float16>(), L.bqk.as<float>(), s);
    }
  }
  JANUS_HIP(hipStreamSynchronize(s));
  w->prepared = true;
}

// The int8 copies of the encoder's linear weights: each output row of the fp32 parameter
// quantised on its own (the fused QKV weight row by row of its three parts).
static void prepare_i8(janus_whisper* w, hipStream_t s) {
  if (w->i8_prepared) return;
  const auto& c = w->cfg;
  const int d = c.d_model, ff = 4 * d;
  const ParamStore& P = w->params;
  auto quant = [&](const std::string& name, int rows, int cols, int8_t* q, float* sc) {
    if (P.has(name)) {
      quant_rows_f32_i8_launch(P.get(name, (int64_t)rows * cols), cols, q, cols, sc, rows, cols, s);
    } else {  // as fuse_f16: a missing part is zeros (scale 0: the product is 0 either way)
      JANUS_HIP(hipMemsetAsync(q, 0, (size_t)rows * cols, s));
      JANUS_HIP(hipMemsetAsync(sc, 0, sizeof(float) * rows, s));
    }
  };
  for (int l = 0; l < c.enc_layers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    EncLayer& L = w->enc[l];
    L.qqkv.ensure((size_t)3 * d * d); L.sqkv.ensure(sizeof(float) * 3 * d);
    L.qo.ensure((size_t)d * d);       L.so.ensure(sizeof(float) * d);
    L.q1.ensure((size_t)ff * d);      L.s1.ensure(sizeof(float) * ff);
    L.q2.ensure((size_t)d * ff);      L.s2.ensure(sizeof(float) * d);
    const char* part[3] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight"};
    for (int i = 0; i < 3; ++i)
      quant(p + part[i], d, d, L.qqkv.as<int8_t>() + (int64_t)i * d * d, L.sqkv.as<float>() + i * d);
    quant(p + "self_attn.out_proj.weight", d, d, L.qo.as<int8_t>(), L.so.as<float>());
    quant(p + "fc1.weight", ff, d, L.q1.as<int8_t>(), L.s1.as<float>());
    quant(p + "fc2.weight", d, ff, L.q2.as<int8_t>(), L.s2.as<float>());
  }
  JANUS_HIP(hipStreamSynchronize(s));
  w->i8_prepared = true;
}

// The int8 copies of the decoder's weights (janus_whisper_set_decoder_compute): every matrix the
// decode call multiplies, quantised per output row from its prepared fp16 copy — the absorbed
// query weight from its absorbed form — and the token embedding as the vocabulary table.
void prepare_dec_i8(janus_whisper* w, hipStream_t s) {
  if (w->dec_i8_prepared) return;
  const auto& c = w->cfg;
  JANUS_CHECK(xattn_supported(c.d_model, c.n_heads), "int8 decoder weights: no absorbed cross-attention at this shape");
  int64_t N, K;
  for (int l = 0; l < c.dec_layers; ++l) {
    DecLayer& L = w->dec[l];
    for (int i = 0; i < 7; ++i) {
      dec_weight_shape(c, i, &N, &K);
      L.q8[i].ensure((size_t)N * K);
      L.s8[i].ensure(sizeof(float) * N);
      quant_weight_rows_i8_launch(L.w16(i).as<_Float16>(), K, L.q8[i].as<int8_t>(), K, L.s8[i].as<float>(), (int)N,
                                  (int)K, s);
    }
  }
  dec_weight_shape(c, -1, &N, &K);
  w->tokq.ensure((size_t)N * K);
  w->toks.ensure(sizeof(float) * N);
  quant_weight_rows_i8_launch(w->tok16.as<_Float16>(), K, w->tokq.as<int8_t>(), K, w->toks.as<float>(), (int)N, (int)K, s);
  JANUS_HIP(hipStreamSynchronize(s));
  w->dec_i8_prepared = true;
}

// The encoder's projections (M = B * 1500 rows): gemm_launch dispatches them to the
// 256 x 256-tile LDS-DMA kernel (gemm_big.hip) when N % 256 == 0 (base.en: every one).
static void enc_gemm(int epi, const GemmArgs& g, hipStream_t s) { gemm_launch(epi, g, s); }

static void encode(janus_whisper* w, const _Float16* mel, int B, _Float16* out, hipStream_t s) {
  const auto& c = w->cfg;
  const int d = c.d_model, H = c.n_heads, Tm = 2 * c.n_audio_ctx, Te = c.n_audio_ctx;
  const int64_t M = (int64_t)B * Te;
  JANUS_CHECK(M < (1ll << 31), "encode: batch too large");
  w->ws_x1.ensure(sizeof(_Float16) * B * Tm * d);
  w->ws_x2.ensure(sizeof(_Float16) * M * d);
  w->ws_r.ensure(sizeof(float) * M * d);
  w->ws_a.ensure(sizeof(_Float16) * M * d);
  w->ws_qkv.ensure(sizeof(_Float16) * M * 3 * d);
  w->ws_o.ensure(sizeof(_Float16) * M * d);
  w->ws_f.ensure(sizeof(_Float16) * M * 4 * d);
  _Float16 *x1 = w->ws_x1.as<_Float16>(), *x2 = w->ws_x2.as<_Float16>();
  float* r = w->ws_r.as<float>();
  _Float16 *a = w->ws_a.as<_Float16>(), *qkv = w->ws_qkv.as<_Float16>(), *o = w->ws_o.as<_Float16>(),
           *f = w->ws_f.as<_Float16>();

  ConvArgs ca{};
  ca.in = mel; ca.in_bs = (int64_t)Tm * c.n_mels; ca.T_in = Tm; ca.Cin = c.n_mels;
  ca.w = w->conv1p.as<_Float16>(); ca.bias = w->params.get("encoder.conv1.bias", d);
  ca.out = x1; ca.out_bs = (int64_t)Tm * d; ca.T_out = Tm; ca.Cout = d;
  ca.res = nullptr; ca.res_bs = 0;
  ca.taps = 3; ca.dil = 1; ca.in_stride = 1; ca.in_off = -1; ca.out_stride = 1; ca.out_off = 0;
  ca.n_rows = Tm; ca.phases = 1; ca.pre_act = ACT_NONE; ca.post_act = ACT_GELU;
  ca.out_scale = 1.0f; ca.accumulate = 0; ca.B = B;
  conv_launch(ca, s);
  ConvArgs cb = ca;
  cb.in = x1; cb.in_bs = (int64_t)Tm * d; cb.T_in = Tm; cb.Cin = d;
  cb.w = w->conv2p.as<_Float16>(); cb.bias = w->params.get("encoder.conv2.bias", d);
  cb.out = x2; cb.out_bs = (int64_t)Te * d; cb.T_out = Te; cb.n_rows = Te; cb.in_stride = 2;
  cb.res = w->pos16.as<_Float16>(); cb.res_bs = 0;
  conv_launch(cb, s);
  cast_f16_f32_launch(x2, r, M * d, s);

  const float scale = 0.125f;  // head_dim 64 ** -0.5
  if (w->enc_compute == JANUS_ENC_COMPUTE_INT8) {
    // the four projections of every layer on the i8 MFMA: their fp16 inputs quantised per
    // row (the LayerNorm outputs in the LayerNorm's own pass), everything else as below
    w->ws_q8.ensure((size_t)M * 4 * d);
    w->ws_qs.ensure(sizeof(float) * M);
    int8_t* q8 = w->ws_q8.as<int8_t>();
    float* qs = w->ws_qs.as<float>();
    auto gemm8 = [&](int epi, int64_t K, const DevMem& W, const DevMem& ws, const float* bias, void* C,
                     int64_t N, const float* R) {
      GemmI8Args g;
      g.A = reinterpret_cast<const signed char*>(q8); g.lda = K;
      g.W = W.as<signed char>(); g.ldw = K;
      g.a_scale = qs; g.w_scale = ws.as<float>(); g.bias = bias;
      g.C = C; g.ldc = N; g.R = R; g.ldr = N; g.M = (int)M; g.N = (int)N; g.K = (int)K;
      gemm_i8_launch(epi, g, s);
    };
    for (int l = 0; l < c.enc_layers; ++l) {
      EncLayer& L = w->enc[l];
      layernorm_quant_i8_launch(r, L.ln1g, L.ln1b, q8, qs, (int)M, d, 1e-5f, s);
      gemm8(EPI_F16, d, L.qqkv, L.sqkv, L.bqkv.as<float>(), qkv, 3 * d, nullptr);
      attention_launch(qkv, o, B, Te, H, scale, s);
      quant_rows_i8_launch(o, d, q8, d, qs, (int)M, d, s);
      gemm8(EPI_RESID_F32, d, L.qo, L.so, L.bo, r, d, r);
      layernorm_quant_i8_launch(r, L.ln2g, L.ln2b, q8, qs, (int)M, d, 1e-5f, s);
      gemm8(EPI_GELU_F16, d, L.q1, L.s1, L.b1, f, 4 * d, nullptr);
      quant_rows_i8_launch(f, 4 * d, q8, 4 * d, qs, (int)M, 4 * d, s);
      gemm8(EPI_RESID_F32, 4 * d, L.q2, L.s2, L.b2, r, d, r);
    }
    layernorm_launch(r, w->params.get("encoder.layer_norm.weight", d),
                     w->params.get("encoder.layer_norm.bias", d), out, (int)M, d, 1e-5f, s);
    return;
  }
  for (int l = 0; l < c.enc_layers; ++l) {
    EncLayer& L = w->enc[l];
    layernorm_launch(r, L.ln1g, L.ln1b, a, (int)M, d, 1e-5f, s);
    enc_gemm(EPI_F16, gargs(a, d, L.wqkv.as<_Float16>(), d, L.bqkv.as<float>(), qkv, 3 * d, (int)M, 3 * d, d), s);
    attention_launch(qkv, o, B, Te, H, scale, s);
    enc_gemm(EPI_RESID_F32, gargs(o, d, L.wo.as<_Float16>(), d, L.bo, r, d, (int)M, d, d, r, d), s);
    layernorm_launch(r, L.ln2g, L.ln2b, a, (int)M, d, 1e-5f, s);
    enc_gemm(EPI_GELU_F16, gargs(a, d, L.w1.as<_Float16>(), d, L.b1, f, 4 * d, (int)M, 4 * d, d), s);
    enc_gemm(EPI_RESID_F32, gargs(f, 4 * d, L.w2.as<_Float16>(), 4 * d, L.b2, r, d, (int)M, d, 4 * d, r, d), s);
  }
  layernorm_launch(r, w->params.get("encoder.layer_norm.weight", d),
                   w->params.get("encoder.layer_norm.bias", d), out, (int)M, d, 1e-5f, s);
}

}  // namespace janus

using namespace janus;

extern "C" int janus_whisper_create(const janus_whisper_config* cfg, janus_whisper** out) {
  return guarded([&] {
    JANUS_CHECK(cfg && out, "null argument");
    JANUS_CHECK(cfg->d_model % 64 == 0 && cfg->n_heads * 64 == cfg->d_model,
                "whisper: head_dim must be 64");
    JANUS_CHECK(cfg->n_mels == 80 || cfg->n_mels == 128, "whisper: 80 or 128 mel bins supported");
    auto* w = new janus_whisper();
    w->cfg = *cfg;
    *out = w;
  });
}

extern "C" int janus_whisper_destroy(janus_whisper* w) {
  return guarded([&] {
    if (w) {
      (void)hipDeviceSynchronize();
      delete w;
    }
  });
}

extern "C" int janus_whisper_set_tensor(janus_whisper* w, const char* name, const float* host,
                                        int64_t numel) {
  return guarded([&] {
    JANUS_CHECK(w && name && host && numel > 0, "bad argument");
    std::lock_guard<std::mutex> lk(w->mu);
    w->params.set(name, host, numel);
    w->prepared = false;
  });
}

static void logmel_frames(janus_whisper* w, const float* pcm, const int64_t* offsets, int batch,
                          int decim, int frames, float* logmel, uint16_t* mel, hipStream_t s) {
  const int nm = w->cfg.n_mels;
  float* lm = logmel;
  if (!lm) {
    w->ws_logmel.ensure(sizeof(float) * (int64_t)batch * frames * nm);
    lm = w->ws_logmel.as<float>();
  }
  w->ws_maxkey.ensure(sizeof(uint32_t) * (batch > 0 ? batch : 1));
  mel_launch(pcm, offsets, batch, w->params.get("mel.basis", 400 * 416),
             w->params.get("mel.filters", 208 * nm), lm, w->ws_maxkey.as<uint32_t>(), frames,
             decim, s, nm);
  mel_normalize_launch(lm, w->ws_maxkey.as<uint32_t>(), reinterpret_cast<_Float16*>(mel), offsets,
                       decim, batch, frames, nm, nm, s);
}

extern "C" int janus_whisper_logmel(janus_whisper* w, const float* pcm, const int64_t* offsets,
                                    int batch, int decim, float* logmel, uint16_t* mel,
                                    void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && pcm && offsets && mel, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    logmel_frames(w, pcm, offsets, batch, decim, 2 * w->cfg.n_audio_ctx, logmel, mel,
                  (hipStream_t)stream);
  });
}

extern "C" int janus_whisper_logmel_frames(janus_whisper* w, const float* pcm,
                                           const int64_t* offsets, int batch, int decim,
                                           int frames, uint16_t* mel, void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && pcm && offsets && mel, "null argument");
    JANUS_CHECK(frames >= 1 && (int64_t)batch * frames * w->cfg.n_mels < (1ll << 40), "bad frame count");
    std::lock_guard<std::mutex> lk(w->mu);
    logmel_frames(w, pcm, offsets, batch, decim, frames, nullptr, mel, (hipStream_t)stream);
  });
}

extern "C" int janus_whisper_encode(janus_whisper* w, const uint16_t* mel, int batch, uint16_t* enc,
                                    void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && mel && enc, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    hipStream_t s = (hipStream_t)stream;
    prepare(w, s);
    if (w->enc_compute == JANUS_ENC_COMPUTE_INT8) prepare_i8(w, s);
    encode(w, reinterpret_cast<const _Float16*>(mel), batch, reinterpret_cast<_Float16*>(enc), s);
  });
}

extern "C" int janus_whisper_set_encoder_compute(janus_whisper* w, int mode) {
  return guarded([&] {
    JANUS_CHECK(w, "null argument");
    JANUS_CHECK(mode == JANUS_ENC_COMPUTE_F16 || mode == JANUS_ENC_COMPUTE_INT8,
                "encoder compute: 0 (float16) or 1 (int8)");
    if (mode == JANUS_ENC_COMPUTE_INT8)
      JANUS_CHECK(w->cfg.d_model % 128 == 0, "int8 encoder: d_model must be a multiple of 128");
    std::lock_guard<std::mutex> lk(w->mu);
    w->enc_compute = mode;
  });
}

extern "C" int janus_whisper_encoder_compute(janus_whisper* w, int32_t* mode) {
  return guarded([&] {
    JANUS_CHECK(w && mode, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    *mode = w->enc_compute;
  });
}

extern "C" int janus_whisper_set_cross_compute(janus_whisper* w, int mode) {
  return guarded([&] {
    JANUS_CHECK(w, "null argument");
    JANUS_CHECK(mode == JANUS_CROSS_COMPUTE_F16 || mode == JANUS_CROSS_COMPUTE_INT8,
                "cross compute: 0 (float16) or 1 (int8)");
    if (mode == JANUS_CROSS_COMPUTE_INT8)
      JANUS_CHECK(xattn_supported(w->cfg.d_model, w->cfg.n_heads),
                  "int8 cross-attention: d_model must be 384, 512, 768, 1024 or 1280 with 64-wide heads");
    std::lock_guard<std::mutex> lk(w->mu);
    w->cross_compute = mode;
  });
}

extern "C" int janus_whisper_cross_compute(janus_whisper* w, int32_t* mode) {
  return guarded([&] {
    JANUS_CHECK(w && mode, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    *mode = w->cross_compute;
  });
}

extern "C" int janus_whisper_set_decoder_compute(janus_whisper* w, int mode) {
  return guarded([&] {
    JANUS_CHECK(w, "null argument");
    JANUS_CHECK(mode == JANUS_DEC_COMPUTE_F16 || mode == JANUS_DEC_COMPUTE_INT8,
                "decoder compute: 0 (float16) or 1 (int8)");
    if (mode == JANUS_DEC_COMPUTE_INT8)
      JANUS_CHECK(xattn_supported(w->cfg.d_model, w->cfg.n_heads),
                  "int8 decoder weights: d_model must be 384, 512, 768, 1024 or 1280 with 64-wide heads");
    std::lock_guard<std::mutex> lk(w->mu);
    // (as the cross mode: the plan's key word keeps the two modes' captured graphs apart, so a
    // call after a switch never replays the other mode's launches)
    w->dec_compute = mode;
  });
}

extern "C" int janus_whisper_decoder_compute(janus_whisper* w, int32_t* mode) {
  return guarded([&] {
    JANUS_CHECK(w && mode, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    *mode = w->dec_compute;
  });
}

extern "C" int janus_whisper_decoder_weight_i8(janus_whisper* w, int layer, int which, int8_t* q_out, float* s_out) {
  return guarded([&] {
    JANUS_CHECK(w && q_out && s_out, "null argument");
    JANUS_CHECK(layer >= -1 && layer < w->cfg.dec_layers, "decoder_weight_i8: layer must be -1 .. dec_layers - 1");
    JANUS_CHECK(layer < 0 || (which >= 0 && which < 7), "decoder_weight_i8: which must be a JANUS_DEC_W_*");
    std::lock_guard<std::mutex> lk(w->mu);
    prepare(w, nullptr);
    prepare_dec_i8(w, nullptr);
    int64_t N, K;
    dec_weight_shape(w->cfg, layer < 0 ? -1 : which, &N, &K);
    const DevMem& q = layer < 0 ? w->tokq : w->dec[layer].q8[which];
    const DevMem& sc = layer < 0 ? w->toks : w->dec[layer].s8[which];
    JANUS_HIP(hipMemcpy(q_out, q.p, (size_t)N * K, hipMemcpyDeviceToHost));
    JANUS_HIP(hipMemcpy(s_out, sc.p, sizeof(float) * N, hipMemcpyDeviceToHost));
  });
}

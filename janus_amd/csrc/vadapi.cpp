// C-ABI of the neural speech gate (vad.hip): a parameter context holding the silero-vad
// v5 16 kHz weights by their published state-dict names; per-channel state lives in
// caller buffers so one context serves any number of channels.
#include <algorithm>
#include <mutex>
#include <vector>
#include "devmem.h"
#include "kernels.h"
#include "../../include/janus.h"


struct janus_vad {
  janus::ParamStore params;
  // janus_vad_probs: gate pre-activations of one pass, carried (h, c), offsets (grow-only)
  janus::DevMem pre, hc, meta;
  std::vector<int64_t> meta_host;
  std::mutex mu;
};

using namespace janus;

// The graph's parameters by their published names (sizes checked).
static VadWeights vad_weights(const ParamStore& P) {
  const std::string m = "_model.";
  VadWeights W;
  W.basis = P.get(m + "stft.forward_basis_buffer", 258 * 256);
  W.w0 = P.get(m + "encoder.0.reparam_conv.weight", 128 * 129 * 3);
  W.b0 = P.get(m + "encoder.0.reparam_conv.bias", 128);
  W.w1 = P.get(m + "encoder.1.reparam_conv.weight", 64 * 128 * 3);
  W.b1 = P.get(m + "encoder.1.reparam_conv.bias", 64);
  W.w2 = P.get(m + "encoder.2.reparam_conv.weight", 64 * 64 * 3);
  W.b2 = P.get(m + "encoder.2.reparam_conv.bias", 64);
  W.w3 = P.get(m + "encoder.3.reparam_conv.weight", 128 * 64 * 3);
  W.b3 = P.get(m + "encoder.3.reparam_conv.bias", 128);
  W.wih = P.get(m + "decoder.rnn.weight_ih", 512 * 128);
  W.whh = P.get(m + "decoder.rnn.weight_hh", 512 * 128);
  W.bih = P.get(m + "decoder.rnn.bias_ih", 512);
  W.bhh = P.get(m + "decoder.rnn.bias_hh", 512);
  W.wo = P.get(m + "decoder.decoder.2.weight", 128);
  W.bo = P.get(m + "decoder.decoder.2.bias", 1);
  return W;
}

extern "C" int janus_vad_create(janus_vad** out) {
  return guarded([&] {
    JANUS_CHECK(out, "null argument");
    *out = new janus_vad();
  });
}

extern "C" int janus_vad_destroy(janus_vad* v) {
  return guarded([&] {
    if (v) {
      (void)hipDeviceSynchronize();
      delete v;
    }
  });
}

extern "C" int janus_vad_set_tensor(janus_vad* v, const char* name, const float* host, int64_t numel) {
  return guarded([&] {
    JANUS_CHECK(v && name && host && numel > 0, "bad argument");
    std::lock_guard<std::mutex> lk(v->mu);
    v->params.set(name, host, numel);
  });
}

extern "C" int janus_vad_run(janus_vad* v, const float* pcm, int n_streams, int n_chunks,
                             int chunk_len, int decim, float* ctx_state, float* hc_state,
                             float* prob, void* stream) {
  return guarded([&] {
    JANUS_CHECK(v && (pcm || n_streams * n_chunks == 0) && ctx_state && hc_state && prob,
                "null argument");
    JANUS_CHECK(n_streams >= 0 && n_chunks >= 0 && decim >= 1, "bad VAD geometry");
    std::lock_guard<std::mutex> lk(v->mu);
    const VadWeights W = vad_weights(v->params);
    silero_vad_launch(pcm, n_streams, n_chunks, chunk_len, decim, W, ctx_state, hc_state, prob,
                      (hipStream_t)stream);
  });
}

// Workspace of a pass when the caller leaves the pass size open: 16384 chunks of
// pre-activations (2 KB each) = 32 MB over all streams, and at least one encoder tile each.
static constexpr int64_t kVadPassBudget = 16384;

extern "C" int janus_vad_probs(janus_vad* v, const float* pcm, const int64_t* offsets, int n_streams,
                               int max_chunks_per_pass, float* prob, void* stream) {
  return guarded([&] {
    JANUS_CHECK(v && n_streams >= 0 && max_chunks_per_pass >= 0, "bad argument");
    if (n_streams == 0) return;
    JANUS_CHECK(offsets && prob, "null argument");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(v->mu);
    const VadWeights W = vad_weights(v->params);
    // [offsets | chunk prefix sums]; stream s of L samples has L / 512 + 1 chunks
    std::vector<int64_t>& mh = v->meta_host;
    mh.assign(2 * (size_t)(n_streams + 1), 0);
    int64_t max_chunks = 0;
    for (int i = 0; i < n_streams; ++i) {
      const int64_t L = offsets[i + 1] - offsets[i];
      JANUS_CHECK(L >= 0, "vad: offsets must not decrease");
      const int64_t n = L / 512 + 1;
      max_chunks = std::max(max_chunks, n);
      mh[n_streams + 1 + i + 1] = mh[n_streams + 1 + i] + n;
    }
    for (int i = 0; i <= n_streams; ++i) mh[i] = offsets[i];
    JANUS_CHECK(pcm || offsets[n_streams] == offsets[0], "null argument");
    int64_t pass = max_chunks_per_pass;
    if (pass == 0) pass = std::max<int64_t>(16, kVadPassBudget / n_streams / 16 * 16);
    pass = std::min(pass, max_chunks);
    v->meta.ensure(sizeof(int64_t) * mh.size());
    v->pre.ensure(sizeof(float) * 512 * (size_t)pass * n_streams);
    v->hc.ensure(sizeof(float) * 256 * (size_t)n_streams);
    // pageable source: staged before the call returns; meta_host lives in the context
    JANUS_HIP(hipMemcpyAsync(v->meta.p, mh.data(), sizeof(int64_t) * mh.size(), hipMemcpyHostToDevice, s));
    const int64_t* d_off = v->meta.as<int64_t>();
    silero_vad_file_launch(pcm, d_off, d_off + n_streams + 1, n_streams, max_chunks, (int)pass, W,
                           v->pre.as<float>(), v->hc.as<float>(), prob, s);
  });
}

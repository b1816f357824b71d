// Language identification head (janus_whisper_detect_language, include/janus.h): the final
// LayerNorm of one decoder position's residual row, the logits of the n_lang language tokens
// alone against the tied token embedding, an fp32 softmax over them and the argmax. One block
// per row. It reads n_lang x d x 2 bytes of the embedding (99 languages: 76 KB at d = 384,
// 152 KB at d = 768) where the full vocabulary projection reads 40 - 80 MB and would filter
// out ~51 800 columns. No atomics, no MFMA: n_lang dot products of length d per row.
#include "mfma.h"
#include "kernels.h"

namespace janus {

constexpr int kLangMax = 128;      // language tokens of one call (Whisper has 99 / 100)
constexpr int kLangMaxD = 2048;    // d_model the LDS row holds

// x [rows][d] fp32 residual rows; g, b [d] the final LayerNorm; emb [n_vocab][d] fp16;
// probs [rows][n_lang] fp32; best [rows] int32 (lowest index on ties).
__global__ __launch_bounds__(256) void lang_head_kernel(
    const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
    const _Float16* __restrict__ emb, int d, int lang_begin, int n_lang, float eps,
    float* __restrict__ probs, int32_t* __restrict__ best) {
  __shared__ __attribute__((aligned(16))) float y[kLangMaxD];   // the normalised row, fp32
  __shared__ float lg[kLangMax];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const float* xr = x + (int64_t)row * d;
  // LayerNorm, two passes in fp32 (norm.hip): every wave reduces the whole row itself, so
  // all four hold the same statistics without a block reduction
  float s = 0.f;
  for (int i = lane; i < d; i += 64) s += xr[i];
  s = wave_sum_f32(s);
  const float mean = s / d;
  float q = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float c = xr[i] - mean;
    q += c * c;
  }
  q = wave_sum_f32(q);
  const float rstd = rsqrtf(q / d + eps);
  for (int i = tid; i < d; i += 256) y[i] = (xr[i] - mean) * rstd * g[i] + b[i];
  __syncthreads();
  // wave w: languages w, w + 4, ...; 16-byte fp16 loads of the embedding row, fp32 FMA
  const int nv = d / 8;
  for (int l = w; l < n_lang; l += 4) {
    const half8* er = reinterpret_cast<const half8*>(emb + (int64_t)(lang_begin + l) * d);
    float acc = 0.f;
    for (int c = lane; c < nv; c += 64) {
      const half8 h = er[c];
      const float4 y0 = *reinterpret_cast<const float4*>(y + 8 * c);
      const float4 y1 = *reinterpret_cast<const float4*>(y + 8 * c + 4);
      acc = fmaf(y0.x, (float)h[0], acc); acc = fmaf(y0.y, (float)h[1], acc);
      acc = fmaf(y0.z, (float)h[2], acc); acc = fmaf(y0.w, (float)h[3], acc);
      acc = fmaf(y1.x, (float)h[4], acc); acc = fmaf(y1.y, (float)h[5], acc);
      acc = fmaf(y1.z, (float)h[6], acc); acc = fmaf(y1.w, (float)h[7], acc);
    }
    acc = wave_sum_f32(acc);
    if (lane == 0) lg[l] = acc;
  }
  __syncthreads();
  // softmax over the n_lang <= 128 logits and their argmax: wave 0, two logits per lane
  if (w != 0) return;
  const float v0 = lane < n_lang ? lg[lane] : -INFINITY;
  const float v1 = lane + 64 < n_lang ? lg[lane + 64] : -INFINITY;
  const float m = wave_max_f32(fmaxf(v0, v1));
  const float e0 = lane < n_lang ? __expf(v0 - m) : 0.f;
  const float e1 = lane + 64 < n_lang ? __expf(v1 - m) : 0.f;
  const float inv = 1.0f / wave_sum_f32(e0 + e1);
  float* pr = probs + (int64_t)row * n_lang;
  if (lane < n_lang) pr[lane] = e0 * inv;
  if (lane + 64 < n_lang) pr[lane + 64] = e1 * inv;
  // the lowest index holding the maximum (lanes without a maximum offer n_lang)
  int idx = v0 == m ? lane : (v1 == m ? lane + 64 : n_lang);
  idx = min(idx, xshfl_i<32>(idx)); idx = min(idx, xshfl_i<16>(idx)); idx = min(idx, xshfl_i<8>(idx));
  idx = min(idx, xshfl_i<4>(idx)); idx = min(idx, xshfl_i<2>(idx)); idx = min(idx, xshfl_i<1>(idx));
  if (lane == 0) best[row] = idx < n_lang ? idx : 0;   // (every logit NaN: no maximum anywhere)
}

void lang_head_launch(const float* x, const float* g, const float* b, const _Float16* emb, int d,
                      int n_vocab, int lang_begin, int n_lang, int rows, float* probs, int32_t* best,
                      hipStream_t s) {
  JANUS_CHECK(n_lang >= 1 && n_lang <= kLangMax, "lang_head: 1 <= n_lang <= 128");
  JANUS_CHECK(d >= 8 && d % 8 == 0 && d <= kLangMaxD, "lang_head: d % 8 == 0, d <= 2048");
  JANUS_CHECK(lang_begin >= 0 && lang_begin + n_lang <= n_vocab, "lang_head: lang_begin + n_lang <= n_vocab");
  JANUS_CHECK(rows >= 1, "lang_head: rows must be >= 1");
  lang_head_kernel<<<rows, 256, 0, s>>>(x, g, b, emb, d, lang_begin, n_lang, 1e-5f, probs, best);
  JANUS_LAUNCH_CHECK();
}

}  // namespace janus

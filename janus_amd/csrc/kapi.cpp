// Kernel-level C-ABI (include/janus_kernels.h): thin wrappers over the launchers.
#include <algorithm>
#include <cstring>
#include <vector>
#include "align.h"
#include "devmem.h"
#include "kernels.h"
#include "decoder.h"
#include "dec_persist.h"
#include "decode_plan.h"
#include "vocoder.h"
#include "../../include/janus_kernels.h"

namespace janus {

// Shared by janus_conv1d_f16 and the vocoder: PyTorch conv hyper-parameters ->
// the implicit-GEMM row mapping of ConvArgs.
ConvArgs conv_args_torch(const _Float16* in, int B, int T_in, int Cin, const _Float16* packed,
                         const float* bias, _Float16* out, int T_out, int Cout, int taps,
                         int stride, int padding, int dilation, int transposed, int pre_act,
                         int post_act, const _Float16* res, int64_t res_bs, float scale,
                         int accumulate) {
  ConvArgs a{};
  a.in = in; a.in_bs = (int64_t)T_in * Cin; a.T_in = T_in; a.Cin = Cin;
  a.w = packed; a.bias = bias;
  a.out = out; a.out_bs = (int64_t)T_out * Cout; a.T_out = T_out; a.Cout = Cout;
  a.res = res; a.res_bs = res_bs;
  a.pre_act = pre_act; a.post_act = post_act; a.out_scale = scale; a.accumulate = accumulate;
  a.B = B;
  if (!transposed) {
    a.taps = taps; a.dil = dilation; a.in_stride = stride; a.in_off = -padding;
    a.out_stride = 1; a.out_off = 0; a.n_rows = T_out; a.phases = 1;
  } else {
    // ConvTranspose1d(k = 2u, stride u, padding p): output t = q*u + ph - p reads input
    // rows q (kernel index ph) and q-1 (kernel index ph+u).
    const int u = stride;
    a.taps = 2; a.dil = -1; a.in_stride = 1; a.in_off = 0;
    a.out_stride = u; a.out_off = -padding; a.phases = u;
    a.n_rows = (T_out + padding) / u + 1;
  }
  return a;
}

}  // namespace janus

using namespace janus;

extern "C" int janus_gemm_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W,
                              int64_t ldw, const float* bias, void* C, int64_t ldc, const float* R,
                              int64_t ldr, int M, int N, int K, void* stream) {
  return guarded([&] {
    GemmArgs g;
    g.A = reinterpret_cast<const _Float16*>(A); g.lda = lda;
    g.W = reinterpret_cast<const _Float16*>(W); g.ldw = ldw;
    g.bias = bias; g.C = C; g.ldc = ldc; g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
    gemm_launch(epi, g, (hipStream_t)stream);
  });
}

extern "C" int janus_gemm_nt128_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W,
                                    int64_t ldw, const float* bias, void* C, int64_t ldc,
                                    const float* R, int64_t ldr, int M, int N, int K, void* stream) {
  return guarded([&] {
    GemmArgs g;
    g.A = reinterpret_cast<const _Float16*>(A); g.lda = lda;
    g.W = reinterpret_cast<const _Float16*>(W); g.ldw = ldw;
    g.bias = bias; g.C = C; g.ldc = ldc; g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
    gemm_nt128_launch(epi, g, (hipStream_t)stream);
  });
}

extern "C" int janus_gemm_lt_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W,
                                 int64_t ldw, const float* bias, void* C, int64_t ldc,
                                 const float* R, int64_t ldr, int M, int N, int K, void* stream) {
  return guarded([&] {
    GemmArgs g;
    g.A = reinterpret_cast<const _Float16*>(A); g.lda = lda;
    g.W = reinterpret_cast<const _Float16*>(W); g.ldw = ldw;
    g.bias = bias; g.C = C; g.ldc = ldc; g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
    JANUS_CHECK(gemm_lt_launch(epi, g, (hipStream_t)stream),
                "gemm_lt: no hipBLASLt plan for this shape / epilogue");
  });
}

extern "C" int janus_gemm_ln_f16(int epi, const float* x, int64_t ldx, const float* gamma,
                                 const float* beta, float eps, const uint16_t* W, int64_t ldw,
                                 const float* bias, void* C, int64_t ldc, int M, int N, int K,
                                 void* stream) {
  return guarded([&] {
    JANUS_CHECK(M <= 64 && K <= 512 && K % 32 == 0, "gemm_ln: M <= 64, K <= 512 (multiple of 32)");
    GemmArgs g;
    g.A = nullptr; g.lda = K; g.R = nullptr; g.ldr = 0;
    g.W = reinterpret_cast<const _Float16*>(W); g.ldw = ldw;
    g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.lnin_x = x; g.lnin_ldx = ldx; g.lnin_g = gamma; g.lnin_b = beta; g.lnin_eps = eps;
    gemm_launch(epi, g, (hipStream_t)stream);
  });
}

extern "C" int janus_resid_ln_f16(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                                  const float* bias, float* x, const float* gamma, const float* beta,
                                  float eps, uint16_t* out, int M, int N, int K, void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && W && x && gamma && beta && out, "resid_ln: null argument");
    ResidLnArgs p;
    p.A = reinterpret_cast<const _Float16*>(A); p.lda = lda;
    p.W = reinterpret_cast<const _Float16*>(W); p.ldw = ldw;
    p.bias = bias; p.x = x; p.ldx = N; p.g = gamma; p.b = beta; p.eps = eps;
    p.out = reinterpret_cast<_Float16*>(out); p.M = M; p.N = N; p.K = K;
    resid_ln_launch(p, (hipStream_t)stream);
  });
}

extern "C" int janus_layernorm_f16(const float* x, const float* gamma, const float* beta,
                                   uint16_t* out, int rows, int d, float eps, void* stream) {
  return guarded([&] {
    layernorm_launch(x, gamma, beta, reinterpret_cast<_Float16*>(out), rows, d, eps,
                     (hipStream_t)stream);
  });
}

extern "C" int janus_quant_rows_i8(const uint16_t* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale,
                                   int M, int K, void* stream) {
  return guarded([&] {
    quant_rows_i8_launch(reinterpret_cast<const _Float16*>(x), ldx, q, ldq, scale, M, K,
                         (hipStream_t)stream);
  });
}

extern "C" int janus_layernorm_quant_i8(const float* x, const float* gamma, const float* beta,
                                        int8_t* q, float* scale, int rows, int d, float eps,
                                        void* stream) {
  return guarded([&] {
    layernorm_quant_i8_launch(x, gamma, beta, q, scale, rows, d, eps, (hipStream_t)stream);
  });
}

extern "C" int janus_gemm_i8(int epi, const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                             const float* a_scale, const float* w_scale, const float* bias, void* C,
                             int64_t ldc, const float* R, int64_t ldr, int M, int N, int K,
                             void* stream) {
  return guarded([&] {
    GemmI8Args g;
    g.A = reinterpret_cast<const signed char*>(A); g.lda = lda;
    g.W = reinterpret_cast<const signed char*>(W); g.ldw = ldw;
    g.a_scale = a_scale; g.w_scale = w_scale; g.bias = bias; g.C = C; g.ldc = ldc;
    g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
    gemm_i8_launch(epi, g, (hipStream_t)stream);
  });
}

extern "C" int janus_quant_weight_rows_i8(const uint16_t* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale,
                                          int M, int K, void* stream) {
  return guarded([&] {
    quant_weight_rows_i8_launch(reinterpret_cast<const _Float16*>(x), ldx, q, ldq, scale, M, K,
                                (hipStream_t)stream);
  });
}

extern "C" int janus_gemm_w8_f16(int epi, const uint16_t* A, int64_t lda, const int8_t* q, const float* scale,
                                 int64_t ldw, const float* bias, void* C, int64_t ldc, const float* R,
                                 int64_t ldr, int M, int N, int K, int a_group_cols, void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && q && scale && C, "gemm_w8: null argument");
    JANUS_CHECK(epi >= EPI_F16 && epi <= EPI_F32, "gemm_w8: epilogues 0 .. 3");
    JANUS_CHECK(epi != EPI_RESID_F32 || R, "gemm_w8: the residual epilogue needs R");
    GemmArgs g;
    g.A = reinterpret_cast<const _Float16*>(A); g.lda = lda;
    g.W = nullptr; g.Wq = q; g.wscale = scale; g.ldw = ldw;
    g.bias = bias; g.C = C; g.ldc = ldc; g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K;
    g.a_group_cols = a_group_cols;
    g.decode_rows = true;   // up to kSkinnyMaxRows rows on the skinny kernel, as a decode step
    gemm_launch(epi, g, (hipStream_t)stream);
  });
}

extern "C" int janus_wave_xor_f32(const float* in, float* out, int n_waves, void* stream) {
  return guarded([&] {
    JANUS_CHECK(in && out, "null argument");
    wave_xor_launch(in, out, n_waves, (hipStream_t)stream);
  });
}

extern "C" int janus_attention_f16(const uint16_t* qkv, uint16_t* out, int batch, int T, int H,
                                   float scale, void* stream) {
  return guarded([&] {
    attention_launch(reinterpret_cast<const _Float16*>(qkv), reinterpret_cast<_Float16*>(out),
                     batch, T, H, scale, (hipStream_t)stream);
  });
}

extern "C" int64_t janus_conv1d_packed_size(int Cin, int Cout, int taps, int transposed,
                                            int stride) {
  const ConvPack g = conv_pack_geometry(Cin, Cout, transposed ? 2 : taps);
  return g.phase_elems * (transposed ? stride : 1);
}

extern "C" int janus_conv1d_pack(const float* w, uint16_t* packed, int Cin, int Cout, int taps,
                                 int transposed, int stride, void* stream) {
  return guarded([&] {
    conv_pack_weights(w, reinterpret_cast<_Float16*>(packed), Cin, Cout, taps, transposed, stride,
                      (hipStream_t)stream);
  });
}

extern "C" int janus_conv1d_f16(const uint16_t* in, int batch, int T_in, int Cin,
                                const uint16_t* packed, const float* bias, uint16_t* out, int T_out,
                                int Cout, int taps, int stride, int padding, int dilation,
                                int transposed, int pre_act, int post_act, const uint16_t* res,
                                int64_t res_bs, float scale, int accumulate, void* stream) {
  return guarded([&] {
    ConvArgs a = conv_args_torch(
        reinterpret_cast<const _Float16*>(in), batch, T_in, Cin,
        reinterpret_cast<const _Float16*>(packed), bias, reinterpret_cast<_Float16*>(out), T_out,
        Cout, taps, stride, padding, dilation, transposed, pre_act, post_act,
        reinterpret_cast<const _Float16*>(res), res_bs, scale, accumulate);
    conv_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_conv1d_f16_ex(const uint16_t* in, int batch, int T_in, int Cin,
                                   const uint16_t* packed, const float* bias, uint16_t* out, int T_out,
                                   int Cout, int taps, int stride, int padding, int dilation,
                                   int transposed, int pre_act, int post_act, const uint16_t* res,
                                   int64_t res_bs, float scale, int accumulate, int post_acc_silu,
                                   int remap, void* stream) {
  return guarded([&] {
    JANUS_CHECK(remap >= -1 && remap <= 3, "conv1d_ex: remap must be -1 .. 3");
    ConvArgs a = conv_args_torch(
        reinterpret_cast<const _Float16*>(in), batch, T_in, Cin,
        reinterpret_cast<const _Float16*>(packed), bias, reinterpret_cast<_Float16*>(out), T_out,
        Cout, taps, stride, padding, dilation, transposed, pre_act, post_act,
        reinterpret_cast<const _Float16*>(res), res_bs, scale, accumulate);
    a.post_acc_silu = post_acc_silu != 0;
    a.remap = remap;
    conv_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_conv_post_f32(const uint16_t* x, int batch, int T, const float* w, float bias,
                                   int pre_silu, float* wav, int16_t* pcm, float* pre_tanh,
                                   void* stream) {
  return guarded([&] {
    JANUS_CHECK(x && w && wav, "null argument");
    conv_post_launch(reinterpret_cast<const _Float16*>(x), batch, T, w, bias, wav, pcm,
                     (hipStream_t)stream, pre_silu != 0, pre_tanh);
  });
}

extern "C" int janus_xcd_remap_i32(int n, int32_t* out, void* stream) {
  return guarded([&] {
    JANUS_CHECK(out, "null argument");
    xcd_remap_launch(n, out, (hipStream_t)stream);
  });
}

extern "C" int janus_resunit_packed_size(int C, int k) { return resunit_kp(C, k) * C; }

extern "C" int janus_resunit_pack(const float* w, uint16_t* packed, int C, int k, void* stream) {
  return guarded([&] {
    resunit_pack(w, reinterpret_cast<_Float16*>(packed), C, k, (hipStream_t)stream);
  });
}

extern "C" int janus_resunit_f16(const uint16_t* x, uint16_t* out, const uint16_t* w1,
                                 const float* b1, const uint16_t* w2, const float* b2, int batch,
                                 int T, int C, int k, int dilation, float scale, int accumulate,
                                 void* stream) {
  return guarded([&] {
    ResUnitArgs a;
    a.x = reinterpret_cast<const _Float16*>(x); a.out = reinterpret_cast<_Float16*>(out);
    a.w1 = reinterpret_cast<const _Float16*>(w1); a.b1 = b1;
    a.w2 = reinterpret_cast<const _Float16*>(w2); a.b2 = b2;
    a.B = batch; a.T = T; a.C = C; a.k = k; a.d = dilation; a.scale = scale;
    a.accumulate = accumulate;
    resunit_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_resunit_f16_ex(const uint16_t* x, uint16_t* out, const uint16_t* w1,
                                    const float* b1, const uint16_t* w2, const float* b2, int batch,
                                    int T, int C, int k, int dilation, float scale, int accumulate,
                                    int post_silu, int max_blocks, void* stream) {
  return guarded([&] {
    ResUnitArgs a;
    a.x = reinterpret_cast<const _Float16*>(x); a.out = reinterpret_cast<_Float16*>(out);
    a.w1 = reinterpret_cast<const _Float16*>(w1); a.b1 = b1;
    a.w2 = reinterpret_cast<const _Float16*>(w2); a.b2 = b2;
    a.B = batch; a.T = T; a.C = C; a.k = k; a.d = dilation; a.scale = scale;
    a.accumulate = accumulate; a.post_silu = post_silu != 0; a.max_blocks = max_blocks;
    resunit_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_cross_attention_f16(const uint16_t* qk, const uint16_t* enc, int batch,
                                         int Te, int D, int H, int nsplit, float* part_c,
                                         float* part_ml, uint16_t* out, void* stream) {
  return guarded([&] {
    XattnArgs a;
    a.qk = reinterpret_cast<const _Float16*>(qk); a.enc = reinterpret_cast<const _Float16*>(enc);
    a.B = batch; a.Te = Te; a.D = D; a.H = H; a.nsplit = nsplit;
    a.part_c = part_c; a.part_ml = part_ml; a.out = reinterpret_cast<_Float16*>(out);
    xattn_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_decode_attention_f16(const uint16_t* q, int64_t q_bs, const uint16_t* k,
                                          const uint16_t* v, int64_t kv_bs, int64_t kv_rs,
                                          int Tkv, uint16_t* out, int64_t o_bs, int batch, int H,
                                          float scale, float* part_o, float* part_ml,
                                          void* stream) {
  return guarded([&] {
    JANUS_CHECK(Tkv <= 512 || (part_o && part_ml), "decode attention: scratch needed past 512 keys");
    decode_attention_split_launch(reinterpret_cast<const _Float16*>(q), q_bs,
                                  reinterpret_cast<const _Float16*>(k),
                                  reinterpret_cast<const _Float16*>(v), kv_bs, kv_rs, Tkv,
                                  reinterpret_cast<_Float16*>(out), o_bs, batch, H, scale, part_o,
                                  part_ml, (hipStream_t)stream);
  });
}

extern "C" int janus_sample_gumbel_f32(const uint32_t* seeds, int batch, int pos, int V, float* out,
                                       void* stream) {
  return guarded([&] {
    JANUS_CHECK(seeds && out, "null argument");
    sample_gumbel_launch(seeds, batch, pos, V, out, (hipStream_t)stream);
  });
}

// ------------------------------------------------------------------ beam search
static DecodeRules beam_rules(int eot, int suppress_blank, int blank, int ts_begin, int no_timestamps,
                              int max_initial_ts) {
  DecodeRules R;
  R.eot = eot; R.suppress_blank = suppress_blank; R.blank = blank; R.ts_begin = ts_begin;
  R.no_timestamps = no_timestamps; R.max_initial_ts = max_initial_ts; R.target = -1; R.inv_temp = 0.f;
  return R;
}

// the vocabulary projection's arguments as the kernel-level entry points give them
static LogitsArgs logits_args(const uint16_t* A, int K, int V, int batch, const DecodeRules& R, const uint8_t* smask,
                              const int32_t* row_rules, int max_blocks, void* parts) {
  LogitsArgs a;
  a.A = reinterpret_cast<const _Float16*>(A); a.lda = K; a.K = K; a.V = V; a.B = batch; a.R = R;
  a.smask = smask; a.rules = reinterpret_cast<const RowRules*>(row_rules);
  a.parts = static_cast<LogitPart*>(parts); a.max_blocks = max_blocks;
  return a;
}

extern "C" int janus_beam_partial_blocks(int V, int K, int max_blocks) {
  return logits_partial_blocks(V, K, max_blocks);
}

extern "C" int janus_beam_logits_topk_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                                          int eot, int suppress_blank, int blank, int ts_begin,
                                          int no_timestamps, int max_initial_ts, const uint8_t* smask,
                                          const int32_t* row_rules, int max_blocks, void* parts,
                                          void* tops, int n2k, float* all_v, int32_t* all_i, float* ts_v,
                                          int32_t* ts_i, void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && W && smask && row_rules && parts && tops && all_v && all_i && ts_v && ts_i, "null argument");
    JANUS_CHECK(batch >= 1 && batch <= kSkinnyMaxRows, "beam_logits_topk: 1 <= batch <= 512");
    static_assert(sizeof(RowRules) == 32 && sizeof(LogitPart) == 56 && sizeof(BeamTop) == 256, "ABI sizes");
    const DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
    const int nblk = logits_partial_blocks(V, K, max_blocks);
    LogitsArgs a = logits_args(A, K, V, batch, R, smask, row_rules, max_blocks, parts);
    a.W = reinterpret_cast<const _Float16*>(W);
    a.tops = static_cast<BeamTop*>(tops);
    logits_partial_launch(a, (hipStream_t)stream);
    beam_rowtop_launch(static_cast<const BeamTop*>(tops), nblk, batch, n2k, all_v, all_i, ts_v, ts_i,
                       (hipStream_t)stream);
  });
}

// The vocabulary projection's partials alone (greedy, or sampling with seeds / inv_temp > 0):
// parts [batch][nblk] LogitPart, nblk = janus_beam_partial_blocks(V, K, max_blocks).
extern "C" int janus_logits_partial_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                                        int eot, int suppress_blank, int blank, int ts_begin,
                                        int no_timestamps, int max_initial_ts, int target,
                                        const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                                        float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                        void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && W && smask && row_rules && parts, "null argument");
    JANUS_CHECK(batch >= 1 && batch <= kSkinnyMaxRows, "logits_partial: 1 <= batch <= 512");
    static_assert(sizeof(RowRules) == 32 && sizeof(LogitPart) == 56, "ABI sizes");
    DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
    R.target = target;
    R.inv_temp = inv_temp > 0.f ? inv_temp : 0.f;
    LogitsArgs a = logits_args(A, K, V, batch, R, smask, row_rules, max_blocks, parts);
    a.W = reinterpret_cast<const _Float16*>(W);
    a.seeds = seeds; a.pos = pos;
    logits_partial_launch(a, (hipStream_t)stream);
  });
}

// ------------------------------------------------------------------ history rules
extern "C" int janus_history_words(int V, int K, int batch) {
  return V >= 1 && batch >= 1 ? (int)history_words(V, K, batch) : 0;
}

extern "C" int janus_history_rules(const int32_t* tokens, int ld, int batch, const int32_t* plen, int n, int V,
                                   int K, int pos0, int n_pos, uint32_t* hist, void* stream) {
  return guarded([&] {
    JANUS_CHECK(tokens && plen && hist, "null argument");
    JANUS_CHECK(batch >= 1 && batch <= kSkinnyMaxRows, "history_rules: 1 <= batch <= 512");
    JANUS_CHECK(pos0 >= 0 && n_pos >= 1 && pos0 + n_pos <= ld, "history_rules: positions outside the token rows");
    for (int pos = pos0; pos < pos0 + n_pos; ++pos)
      history_rules_launch(tokens, ld, pos, plen, n, V, logits_row_group(K), hist, batch, (hipStream_t)stream);
  });
}

extern "C" int janus_logits_partial_hist_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                                             int eot, int suppress_blank, int blank, int ts_begin,
                                             int no_timestamps, int max_initial_ts, int target,
                                             const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                                             float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                             const uint32_t* hist, float repetition_penalty, void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && W && smask && row_rules && parts && hist, "null argument");
    JANUS_CHECK(batch >= 1 && batch <= kSkinnyMaxRows, "logits_partial: 1 <= batch <= 512");
    JANUS_CHECK(repetition_penalty > 0.f, "logits_partial_hist: repetition_penalty must be > 0");
    DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
    R.target = target;
    R.inv_temp = inv_temp > 0.f ? inv_temp : 0.f;
    LogitsArgs a = logits_args(A, K, V, batch, R, smask, row_rules, max_blocks, parts);
    a.W = reinterpret_cast<const _Float16*>(W);
    a.seeds = seeds; a.pos = pos;
    a.hist = hist; a.rep_pen = repetition_penalty;
    logits_partial_launch(a, (hipStream_t)stream);
  });
}

static int logits_partial_w8(const uint16_t* A, const int8_t* q, const float* scale, int K, int V, int batch,
                             const DecodeRules& R, const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                             const uint32_t* seeds, int pos, void* parts, const uint32_t* hist,
                             float repetition_penalty, void* stream) {
  return guarded([&] {
    JANUS_CHECK(A && q && scale && smask && row_rules && parts, "null argument");
    JANUS_CHECK(batch >= 1 && batch <= kSkinnyMaxRows, "logits_partial: 1 <= batch <= 512");
    LogitsArgs a = logits_args(A, K, V, batch, R, smask, row_rules, max_blocks, parts);
    a.Wq = q; a.wscale = scale;
    a.seeds = seeds; a.pos = pos;
    a.hist = hist; a.rep_pen = repetition_penalty;
    logits_partial_launch(a, (hipStream_t)stream);
  });
}

extern "C" int janus_logits_partial_w8_f16(const uint16_t* A, const int8_t* q, const float* scale, int K, int V,
                                           int batch, int eot, int suppress_blank, int blank, int ts_begin,
                                           int no_timestamps, int max_initial_ts, int target,
                                           const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                                           float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                           void* stream) {
  DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
  R.target = target;
  R.inv_temp = inv_temp > 0.f ? inv_temp : 0.f;
  return logits_partial_w8(A, q, scale, K, V, batch, R, smask, row_rules, max_blocks, seeds, pos, parts, nullptr,
                           1.f, stream);
}

extern "C" int janus_logits_partial_hist_w8_f16(const uint16_t* A, const int8_t* q, const float* scale, int K,
                                                int V, int batch, int eot, int suppress_blank, int blank,
                                                int ts_begin, int no_timestamps, int max_initial_ts, int target,
                                                const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                                                float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                                const uint32_t* hist, float repetition_penalty, void* stream) {
  if (!hist || !(repetition_penalty > 0.f)) {
    set_error("logits_partial_hist_w8: hist must be non-null and repetition_penalty > 0");
    return -1;
  }
  DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
  R.target = target;
  R.inv_temp = inv_temp > 0.f ? inv_temp : 0.f;
  return logits_partial_w8(A, q, scale, K, V, batch, R, smask, row_rules, max_blocks, seeds, pos, parts, hist,
                           repetition_penalty, stream);
}

extern "C" int janus_beam_step(const void* parts, const void* tops, int nblk, int eot, int suppress_blank,
                               int blank, int ts_begin, int no_timestamps, int max_initial_ts,
                               int32_t* row_rules, int32_t* tokens, int ld, int pos, int32_t* done,
                               float* sum_lp, int32_t* n_tok, const int32_t* plen, int beam_size,
                               int n_windows, int32_t* nlive, int32_t* nfin, int32_t* wdone,
                               int32_t* moved, int32_t* parent, int32_t* fin_tok, float* fin_s,
                               int32_t* fin_n, void* stream) {
  return guarded([&] {
    JANUS_CHECK(parts && tops && row_rules && tokens && done && sum_lp && n_tok && plen && nlive && nfin &&
                    wdone && moved && parent && fin_tok && fin_s && fin_n, "null argument");
    JANUS_CHECK(n_windows >= 1, "beam_step: n_windows must be >= 1");
    const DecodeRules R = beam_rules(eot, suppress_blank, blank, ts_begin, no_timestamps, max_initial_ts);
    BeamState st{};
    st.k = beam_size; st.length_penalty = 1.0f;
    st.nlive = nlive; st.nfin = nfin; st.wdone = wdone; st.moved = moved; st.parent = parent;
    st.fin_tok = fin_tok; st.fin_s = fin_s; st.fin_n = fin_n;
    SelectArgs a;
    a.parts = static_cast<const LogitPart*>(parts); a.nblk = nblk; a.R = R;
    a.rules = reinterpret_cast<RowRules*>(row_rules); a.tokens = tokens; a.ld = ld; a.pos = pos;
    a.done = done; a.sum_lp = sum_lp; a.n_tok = n_tok; a.plen = plen;
    beam_step_launch(a, static_cast<const BeamTop*>(tops), st, n_windows, (hipStream_t)stream);
  });
}

extern "C" int janus_beam_reorder_f16(uint16_t* kc, uint16_t* vc, int layers, int n_windows, int beam_size,
                                      int n_ctx, int d, int pos, const int32_t* parent,
                                      const int32_t* moved, void* stream) {
  return guarded([&] {
    JANUS_CHECK(kc && vc && parent && moved, "null argument");
    beam_reorder_launch(reinterpret_cast<_Float16*>(kc), reinterpret_cast<_Float16*>(vc), layers, n_windows,
                        beam_size, n_ctx, d, pos, parent, moved, (hipStream_t)stream);
  });
}

extern "C" int janus_decode_plan_describe(const janus_whisper_config* cfg, const janus_decode_options* opt,
                                          const janus_decode_rows* rows, int batch, int cus, int resident,
                                          int multi_lane, float temperature, const float* temperatures,
                                          int beam_size, const int32_t* stand, int n_stand, int stand_maxlen,
                                          char* text, int text_cap, int64_t* key, int key_cap, int32_t* n_key) {
  return janus_decode_plan_describe_modes(cfg, opt, rows, batch, cus, resident, multi_lane, temperature,
                                          temperatures, beam_size, stand, n_stand, stand_maxlen,
                                          JANUS_CROSS_COMPUTE_F16, JANUS_DEC_COMPUTE_F16, text, text_cap, key,
                                          key_cap, n_key);
}

extern "C" int janus_decode_plan_describe_cross(const janus_whisper_config* cfg, const janus_decode_options* opt,
                                                const janus_decode_rows* rows, int batch, int cus, int resident,
                                                int multi_lane, float temperature, const float* temperatures,
                                                int beam_size, const int32_t* stand, int n_stand,
                                                int stand_maxlen, int cross_compute, char* text, int text_cap,
                                                int64_t* key, int key_cap, int32_t* n_key) {
  return janus_decode_plan_describe_modes(cfg, opt, rows, batch, cus, resident, multi_lane, temperature,
                                          temperatures, beam_size, stand, n_stand, stand_maxlen, cross_compute,
                                          JANUS_DEC_COMPUTE_F16, text, text_cap, key, key_cap, n_key);
}

extern "C" int janus_decode_plan_describe_modes(const janus_whisper_config* cfg, const janus_decode_options* opt,
                                                const janus_decode_rows* rows, int batch, int cus, int resident,
                                                int multi_lane, float temperature, const float* temperatures,
                                                int beam_size, const int32_t* stand, int n_stand,
                                                int stand_maxlen, int cross_compute, int dec_compute, char* text,
                                                int text_cap, int64_t* key, int key_cap, int32_t* n_key) {
  return guarded([&] {
    JANUS_CHECK(cfg && opt && text && key && n_key, "null argument");
    JANUS_CHECK(batch >= 1, "decode: batch must be >= 1");
    const std::vector<uint32_t> seeds(batch, 0);
    const DecodeSampling smp{temperatures ? 1.0f : temperature, seeds.data(), temperatures};
    const BeamMode bm{beam_size, 1.0f};
    const std::vector<int32_t> st(stand, stand + (stand ? n_stand : 0));
    SegDevice seg;
    seg.grid = [](int B, int n_cus, bool) { return dec_seg_grid(B, n_cus, false); };
    seg.resident = [resident](int, int) { return resident != 0; };
    const DecodePlan P = plan_decode(*cfg, *opt, rows, (temperatures || temperature > 0.f) ? &smp : nullptr,
                                     beam_size > 0 ? &bm : nullptr, batch, cus, multi_lane != 0,
                                     LaneStand{&st, stand_maxlen}, seg, cross_compute, dec_compute);
    const std::string d = P.describe();
    std::vector<int64_t> k;
    P.append_key(k);
    JANUS_CHECK((int)d.size() < text_cap && (int)k.size() <= key_cap, "decode_plan_describe: buffer too small");
    std::memcpy(text, d.c_str(), d.size() + 1);
    std::copy(k.begin(), k.end(), key);
    *n_key = (int32_t)k.size();
  });
}

// ------------------------------------------------------------------ word alignment kernels
namespace {
// a one-window device table for the alignment kernels' test entries
const AlignWinDev* one_window(DevMem& m, int n, int F, int N, hipStream_t s) {
  AlignWinDev W{};
  W.n = n; W.F = F; W.N = N;
  m.ensure(sizeof(W));
  JANUS_HIP(hipMemcpyAsync(m.p, &W, sizeof(W), hipMemcpyHostToDevice, s));
  JANUS_HIP(hipStreamSynchronize(s));   // W is a local
  return m.as<AlignWinDev>();
}
}  // namespace

extern "C" int janus_align_dtw_f32(const float* x, int N, int F, uint8_t* trace, int32_t* text_indices,
                                   int32_t* time_indices, int32_t* path_len, void* stream) {
  return guarded([&] {
    JANUS_CHECK(x && trace && text_indices && time_indices && path_len, "null argument");
    JANUS_CHECK(N >= 1 && N <= 511 && F >= 1 && F <= 4096, "align_dtw: 1 <= N <= 511, 1 <= F <= 4096");
    hipStream_t s = (hipStream_t)stream;
    DevMem win, rev;
    rev.ensure(sizeof(int32_t) * 2 * (size_t)(N + F));
    align_dtw_launch(x, one_window(win, N + 1, F, N, s), 1, 0, trace, rev.as<int32_t>(), text_indices,
                     time_indices, path_len, N + F, s);
    JANUS_HIP(hipStreamSynchronize(s));   // the scratch goes with this call
  });
}

extern "C" int janus_align_reduce_f32(const float* probs, int heads, int n, int F, int sot_len, float* A,
                                      void* stream) {
  return guarded([&] {
    JANUS_CHECK(probs && A, "null argument");
    JANUS_CHECK(heads >= 1 && heads <= kAlignMaxHeads && F >= 1 && F <= 4096 && sot_len >= 0 && n >= sot_len + 2 &&
                    n <= 4096, "align_reduce: 1 .. 64 heads, 1 <= F <= 4096, sot_len + 2 <= n <= 4096");
    hipStream_t s = (hipStream_t)stream;
    DevMem win, stats;
    stats.ensure(sizeof(double) * 2 * (size_t)heads * F);
    align_reduce_launch(probs, one_window(win, n, F, n - sot_len - 1, s), 1, heads, sot_len, n, F,
                        stats.as<double>(), A, s);
    JANUS_HIP(hipStreamSynchronize(s));
  });
}

extern "C" int janus_align_token_prob_f16(const float* x, const float* gamma, const float* beta,
                                          const uint16_t* W, int rows, int d, int V, const int32_t* target,
                                          float* prob, void* stream) {
  return guarded([&] {
    JANUS_CHECK(x && gamma && beta && W && target && prob, "null argument");
    JANUS_CHECK(rows >= 1 && rows <= 4096 && d % 8 == 0 && V >= 1, "align_token_prob: 1 .. 4096 rows, d % 8 == 0");
    hipStream_t s = (hipStream_t)stream;
    const int vpad = (V + 7) & ~7, chunk = 64;
    DevMem a, logits, idx;
    a.ensure(sizeof(_Float16) * (size_t)rows * d);
    logits.ensure(sizeof(float) * (size_t)chunk * vpad);
    std::vector<int32_t> ident(rows);
    for (int r = 0; r < rows; ++r) ident[r] = r;
    idx.ensure(sizeof(int32_t) * rows);
    JANUS_HIP(hipMemcpyAsync(idx.p, ident.data(), sizeof(int32_t) * rows, hipMemcpyHostToDevice, s));
    layernorm_launch(x, gamma, beta, a.as<_Float16>(), rows, d, 1e-5f, s);
    for (int r0 = 0; r0 < rows; r0 += chunk) {   // no [rows][V] logits: one chunk of rows at a time
      const int m = std::min(chunk, rows - r0);
      GemmArgs g;
      g.A = a.as<_Float16>() + (int64_t)r0 * d; g.lda = d;
      g.W = reinterpret_cast<const _Float16*>(W); g.ldw = d;
      g.bias = nullptr; g.C = logits.p; g.ldc = vpad; g.R = nullptr; g.ldr = 0; g.M = m; g.N = V; g.K = d;
      gemm_nt128_launch(EPI_F32, g, s);
      align_rowprob_launch(logits.as<float>(), vpad, V, target + r0, idx.as<int32_t>() + r0, m, prob, s);
    }
    JANUS_HIP(hipStreamSynchronize(s));
  });
}

// ------------------------------------------------------------------ language head
extern "C" int janus_lang_head_f16(const float* x, const float* gamma, const float* beta, const uint16_t* emb,
                                   int d, int lang_begin, int n_lang, int rows, float* probs, int32_t* best,
                                   void* stream) {
  return guarded([&] {
    JANUS_CHECK(x && gamma && beta && emb && probs && best, "null argument");
    JANUS_CHECK(lang_begin >= 0 && n_lang >= 1, "lang_head: lang_begin >= 0, n_lang >= 1");
    // (emb's row count is the caller's: it holds at least lang_begin + n_lang rows)
    lang_head_launch(x, gamma, beta, reinterpret_cast<const _Float16*>(emb), d, lang_begin + n_lang,
                     lang_begin, n_lang, rows, probs, best, (hipStream_t)stream);
  });
}

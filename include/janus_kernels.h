/*
 * janus_kernels.h — kernel-level C-ABI of libjanus_hip.so (gfx950).
 *
 * The building blocks the whisper / vocoder entry points of janus.h are made of,
 * exposed for parity tests and for callers that orchestrate their own graphs. All
 * pointers are [device]; fp16 tensors are uint16_t (binary16 bits); all calls are
 * asynchronous on `stream`. Return 0 on success (janus_last_error() otherwise).
 */
#ifndef JANUS_KERNELS_H_
#define JANUS_KERNELS_H_

#include <stddef.h>
#include <stdint.h>
#include "janus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Epilogues of janus_gemm_f16 */
enum { JANUS_EPI_F16 = 0, JANUS_EPI_GELU_F16 = 1, JANUS_EPI_RESID_F32 = 2, JANUS_EPI_F32 = 3 };
/* Activations of janus_conv1d_f16 */
enum { JANUS_ACT_NONE = 0, JANUS_ACT_SILU = 1, JANUS_ACT_GELU = 2, JANUS_ACT_TANH = 3 };

/*
 * C[M,N] = epi(A[M,K] · W[N,K]^T + bias[N]); A, W fp16 (K contiguous, K % 8 == 0);
 * C fp16 or fp32 by epilogue; JANUS_EPI_RESID_F32: C = R + (A·W^T + bias) in fp32.
 * Replaces the dense projections inside CTranslate2's Whisper (transcriber.py:23-27).
 */
int janus_gemm_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                   const float* bias, void* C, int64_t ldc, const float* R, int64_t ldr, int M,
                   int N, int K, void* stream);

/* The same product on the general 128 x 128-tile kernel (any N, K % 8 == 0). janus_gemm_f16
 * dispatches M > 64 products with N % 256 == 0 and K % 64 == 0 to the 256 x 256-tile
 * kernel (gemm_big.hip, the encoder's projections); both accumulate each output over the
 * same k-steps in the same order, so their results are bit-identical. */
int janus_gemm_nt128_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                         const float* bias, void* C, int64_t ldc, const float* R, int64_t ldr, int M,
                         int N, int K, void* stream);

/* The same product on hipBLASLt — a comparison point for the hand-written kernels
 * (tools/gemm_big_probe.py); no product path calls it. epi F16 / F32 / RESID_F32 (C == R
 * in place) / GELU_F16 (bias epilogue, then an exact-erf GELU pass); bias required;
 * workspace-free plans only. Error when the library has no such plan for the shape. */
int janus_gemm_lt_f16(int epi, const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                      const float* bias, void* C, int64_t ldc, const float* R, int64_t ldr, int M,
                      int N, int K, void* stream);

/* LayerNorm rows of an fp32 [rows][d] tensor into fp16 (eps as given). */
/* C = epilogue(LayerNorm(x) W^T + bias) for M <= 64 rows: the LayerNorm of each block's
 * rows (fp32 x, row stride ldx; gamma/beta f32 [K]; two-pass fp32 statistics) is computed in
 * the GEMM's prologue instead of a separate janus_layernorm_f16 launch. K <= 512, K % 4 == 0;
 * epi one of EPI_F16 / EPI_GELU_F16. The decoder's pre-LN projections (transcriber.py:53-57
 * -> Whisper decoder layers). */
int janus_gemm_ln_f16(int epi, const float* x, int64_t ldx, const float* gamma, const float* beta,
                      float eps, const uint16_t* W, int64_t ldw, const float* bias, void* C,
                      int64_t ldc, int M, int N, int K, void* stream);
int janus_layernorm_f16(const float* x, const float* gamma, const float* beta, uint16_t* out,
                        int rows, int d, float eps, void* stream);

/*
 * Int8 projections (gemm_i8.hip): the encoder's linear layers under
 * janus_whisper_set_encoder_compute(JANUS_ENC_COMPUTE_INT8), CTranslate2's int8 compute type
 * (transcriber.py:23-27, compute_type='int8').
 *
 * Row-wise symmetric quantiser, per row x[0..K): amax = max |x[k]| (exact in fp32);
 * amax == 0: q = 0, scale = 1.0f; otherwise inv = 127.0f / amax (correctly rounded),
 * q[k] = (int8) clamp(rintf(x[k] * inv), -127, 127) (one rounding in the product, ties of
 * rintf to even), scale = amax / 127.0f (correctly rounded).
 * x fp16 [M][K] with row stride ldx -> q int8 [M][K] with row stride ldq, scale f32 [M].
 * K % 16 == 0, K <= 3072, any M.
 */
int janus_quant_rows_i8(const uint16_t* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                        int K, void* stream);
/* janus_layernorm_f16 followed by janus_quant_rows_i8 in one pass over x f32 [rows][d], bit
 * for bit (q int8 [rows][d], scale f32 [rows]); the fp16 row is never written. d % 16 == 0,
 * d <= 2048. */
int janus_layernorm_quant_i8(const float* x, const float* gamma, const float* beta, int8_t* q,
                             float* scale, int rows, int d, float eps, void* stream);
/*
 * C[M,N] = epi( float(sum_k A[m,k] * W[n,k]) * (a_scale[m] * w_scale[n]) + bias[n] ):
 * int8 A [M][K] and W [N][K] (K contiguous), exact int32 accumulation on
 * v_mfma_i32_16x16x64_i8, then in fp32 with one rounding per operation (no fma):
 * s = a_scale[m] * w_scale[n]; y = (float)acc * s + bias[n] (bias may be NULL: 0).
 * epi JANUS_EPI_F32: y; JANUS_EPI_F16: fp16(y); JANUS_EPI_GELU_F16: fp16(gelu(y));
 * JANUS_EPI_RESID_F32: C = R + y (R may alias C). Any M; N % 128 == 0 and K % 128 == 0
 * (an error otherwise); lda, ldw multiples of 16, ldc of 8; 16-byte aligned operands.
 */
int janus_gemm_i8(int epi, const int8_t* A, int64_t lda, const int8_t* W, int64_t ldw,
                  const float* a_scale, const float* w_scale, const float* bias, void* C, int64_t ldc,
                  const float* R, int64_t ldr, int M, int N, int K, void* stream);

/* The cross-lane moves every wave reduction of the library uses (DPP / v_permlane swaps in
 * place of ds_bpermute): in [device] f32 [n_waves][64] -> out [device] f32 [n_waves][6][64],
 * out[w][k][l] = in[w][l ^ (1 << k)] when they are right. Test entry. */
int janus_wave_xor_f32(const float* in, float* out, int n_waves, void* stream);

/* x[M][N] += A[M][K] W[N][K]^T + bias (fp32 residual, in place), then out[M][N] =
 * LayerNorm(x) fp16 (gamma/beta f32 [N], eps) in ONE launch: 16 rows per workgroup over
 * all N columns. N = K in {384, 512} (tiny.en / base.en d_model). Bit-identical to
 * janus_gemm_f16(JANUS_EPI_RESID_F32) at M <= 64 followed by janus_layernorm_f16. The
 * decoder's attention output projections and the LayerNorm after them
 * (transcriber.py:53-57 -> Whisper decoder layers: self_attn.out_proj + encoder_attn_layer_norm,
 * encoder_attn.out_proj + final_layer_norm). */
int janus_resid_ln_f16(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw,
                       const float* bias, float* x, const float* gamma, const float* beta,
                       float eps, uint16_t* out, int M, int N, int K, void* stream);

/* Non-causal multi-head attention, head_dim 64: qkv fp16 [B*T][3*H*64] -> out fp16 [B*T][H*64]. */
int janus_attention_f16(const uint16_t* qkv, uint16_t* out, int batch, int T, int H, float scale,
                        void* stream);

/* Size in fp16 elements of the packed weight buffer janus_conv1d_pack expects/produces. */
int64_t janus_conv1d_packed_size(int Cin, int Cout, int taps, int transposed, int stride);
/*
 * Pack fp32 PyTorch conv weights for janus_conv1d_f16: Conv1d [Cout][Cin][taps]
 * (transposed=0) or ConvTranspose1d [Cin][Cout][2*stride] (transposed=1).
 */
int janus_conv1d_pack(const float* w, uint16_t* packed, int Cin, int Cout, int taps,
                      int transposed, int stride, void* stream);
/*
 * Time-major 1-D convolution on MFMA: in [B][T_in][Cin], out [B][T_out][Cout] (fp16).
 * transposed=0: PyTorch Conv1d(Cin, Cout, taps, stride, padding, dilation)
 * transposed=1: ConvTranspose1d(Cin, Cout, 2*stride, stride, padding) (taps ignored).
 * y = post_act(conv(pre_act(x)) + bias); y += res (fp16 [B][T_out][Cout], may be NULL,
 * res_bs = batch stride in elements, 0 to broadcast); out = (accumulate ? out : 0) + scale*y.
 * (pre_act, post_act) is one of (NONE, NONE), (SILU, NONE), (SILU, SILU), (NONE, GELU) —
 * the pairs of the Whisper stem and the generator, compiled in; others return an error.
 */
int janus_conv1d_f16(const uint16_t* in, int batch, int T_in, int Cin, const uint16_t* packed,
                     const float* bias, uint16_t* out, int T_out, int Cout, int taps, int stride,
                     int padding, int dilation, int transposed, int pre_act, int post_act,
                     const uint16_t* res, int64_t res_bs, float scale, int accumulate,
                     void* stream);
/* Test entry: janus_conv1d_f16 plus the two launcher arguments only the generator sets.
 * post_acc_silu: out = silu(out) after the accumulation; remap: the tile order (0 dispatch
 * order, 1 XCD runs of row blocks, 2 XCD runs over the whole grid, 3 as 2 with the phases of
 * a row block adjacent, -1 the default) — no order changes any value. */
int janus_conv1d_f16_ex(const uint16_t* in, int batch, int T_in, int Cin, const uint16_t* packed,
                        const float* bias, uint16_t* out, int T_out, int Cout, int taps, int stride,
                        int padding, int dilation, int transposed, int pre_act, int post_act,
                        const uint16_t* res, int64_t res_bs, float scale, int accumulate,
                        int post_acc_silu, int remap, void* stream);
/* Test entry: the generator's tail. x fp16 [B][T][16] -> y = b + sum_{c,j} w[c][j] *
 * s(x[t + j - 6][c]) (w f32 [16][13], s = SiLU when pre_silu, else identity; zero outside
 * [0, T)); wav f32 [B][T] = tanh(y), pcm int16 [B][T] = clip(rint(wav * 32767)) (may be
 * NULL), pre_tanh f32 [B][T] = y (may be NULL). */
int janus_conv_post_f32(const uint16_t* x, int batch, int T, const float* w, float bias,
                        int pre_silu, float* wav, int16_t* pcm, float* pre_tanh, void* stream);
/* Test entry: out [device] int32 [n], out[i] = the logical tile that block i of an n-block
 * grid takes (the XCD-aware order of the vocoder and GEMM kernels): a permutation of 0..n-1. */
int janus_xcd_remap_i32(int n, int32_t* out, void* stream);

/*
 * Fused fish-speech ResBlock1 unit (C = 16 or 32 with k in {3, 7, 11} and dilation in
 * {1, 3, 5}; C = 64, 128 or 256 with odd k <= 11 and (k - 1) * dilation <= 50; any other
 * (C, k, dilation) is an error):
 * out = (accumulate ? out : 0) + scale * (x + c2(silu(c1(silu(x)) + b1)) + b2), with
 * c1 = Conv1d(C, C, k, dilation, padding dilation*(k-1)/2), c2 = Conv1d(C, C, k,
 * padding (k-1)/2); x/out fp16 [B][T][C] (must not alias); weights packed by
 * janus_resunit_pack from PyTorch [C][C][k] fp32 into janus_resunit_packed_size halves.
 */
int janus_resunit_packed_size(int C, int k);
int janus_resunit_pack(const float* w, uint16_t* packed, int C, int k, void* stream);
int janus_resunit_f16(const uint16_t* x, uint16_t* out, const uint16_t* w1, const float* b1,
                      const uint16_t* w2, const float* b2, int batch, int T, int C, int k,
                      int dilation, float scale, int accumulate, void* stream);
/* Test entry: janus_resunit_f16 plus post_silu (out = silu(out) after the accumulation) and
 * max_blocks (> 0: at C = 16 / 32 the persistent grid has at most that many blocks, each
 * walking several tiles; ignored at C >= 64). Any max_blocks gives the same bits. */
int janus_resunit_f16_ex(const uint16_t* x, uint16_t* out, const uint16_t* w1, const float* b1,
                         const uint16_t* w2, const float* b2, int batch, int T, int C, int k,
                         int dilation, float scale, int accumulate, int post_silu, int max_blocks,
                         void* stream);

/*
 * Decoder cross-attention over the encoder output with absorbed K/V projections:
 * for every utterance b and head h (H * 64 == D, D in {384, 512, 768, 1024, 1280}),
 *   p = softmax_2(qk[b][h] . enc[b]^T)   (base-2 softmax: qk carries log2(e)/8),
 *   out[b][h*D:(h+1)*D] = p . enc[b]
 * qk fp16 [B][H*D], enc fp16 [B][Te][D], out fp16 [B][H*D]; nsplit key splits
 * (1..63) with scratch part_c f32 [B][nsplit][H][D] and part_ml f32 [B][nsplit][H][2].
 * Replaces the cross-attention K/V projections + attention of the Whisper decoder
 * (transcriber.py:23-27); see janus_amd/csrc/xattn.hip for the re-association.
 */
int janus_cross_attention_f16(const uint16_t* qk, const uint16_t* enc, int batch, int Te, int D,
                              int H, int nsplit, float* part_c, float* part_ml, uint16_t* out,
                              void* stream);

/* Decoder self-attention, one query per (utterance, head) against a KV cache:
 *   out[b][h*64:(h+1)*64] = softmax(q_h . K_h[0:Tkv]^T * scale) . V_h[0:Tkv]
 * q fp16 rows of stride q_bs; k/v fp16 [B][>=Tkv][H*64] with batch stride kv_bs and row
 * stride kv_rs (elements); out fp16 rows of stride o_bs. Tkv <= 512 runs one block per
 * (head, utterance); longer caches split keys over blocks with scratch part_o f32
 * [B][ceil(Tkv/64)][H*64] and part_ml f32 [B][ceil(Tkv/64)][H][2] (may be NULL when
 * Tkv <= 512). The per-step self-attention of the greedy decoder (transcriber.py:53-57
 * -> model.transcribe, CTranslate2 decoder with KV cache). */
int janus_decode_attention_f16(const uint16_t* q, int64_t q_bs, const uint16_t* k,
                               const uint16_t* v, int64_t kv_bs, int64_t kv_rs, int Tkv,
                               uint16_t* out, int64_t o_bs, int batch, int H, float scale,
                               float* part_o, float* part_ml, void* stream);

/* Per segment b of a flat f32 array (offsets[B+1], int64): the count of values > 0 and
 * np.mean of those values in order, numpy float32 bit for bit (float32 pairwise sums over
 * 8192-element buffers, float64 divide by the count, 0 when none). The voiced-f0 mean of
 * janus_prosody_analyze (backend/services/prosody.py:86-90: pitch_values.append(pitch) for
 * pitch > 0, np.mean(pitch_values)) exposed for edge tests. */
int janus_np_voiced_mean_f32(const float* values, const int64_t* offsets, int batch,
                             float* mean_out, int32_t* count_out, void* stream);

/*
 * The decoder's sampling noise (janus_whisper_decode_sample_ex): out [batch][V] f32 =
 * Gumbel(0, 1) draw of token t for row b at position pos, -log(-log u) with u an odd
 * multiple of 2^-24 from a murmur3-finalised hash of (seeds[b] [device uint32], pos, t).
 * Lets tests pin the CPU oracle's noise to the device's.
 */
int janus_sample_gumbel_f32(const uint32_t* seeds, int batch, int pos, int V, float* out,
                            void* stream);

/*
 * Beam search kernels (janus_whisper_decode_beam_ex), one test entry each. Device pointers.
 *
 * janus_beam_partial_blocks: partials per row the vocabulary projection writes for this
 * shape (returns the count, not a status).
 *
 * janus_beam_logits_topk_f16: the beam instantiation of the vocabulary projection —
 * logits = A[batch][K] . W[V][K]^T (fp16, K = 384 / 512 / 768) filtered by the decoding
 * rules (smask: V suppress bytes padded to a multiple of 16; row_rules [batch][8] int32 =
 * sample_begin, suppress_all_ts, suppress_text, ts_floor, last_stamp, 3 pad) with no logits
 * in memory: parts [batch][nblk] x 56 B (m_all, s_all, m_text, m_ts, s_ts, b_all_v, b_all_i,
 * b_ts_v, b_ts_i, t_v, m_raw, s_raw, b_all_r, b_ts_r) and tops [batch][nblk] x 256 B (16
 * logits + 16 indices over every allowed token, then the same over allowed timestamps;
 * sorted, first index on ties, unused = -inf / 0x7fffffff), then merged per row into the
 * best n2k (<= 16) of both sets: all_v / all_i / ts_v / ts_i [batch][n2k] (unused: -inf / -1).
 *
 * janus_beam_step: one selection step of n_windows windows x beam_size rows at position
 * pos from hand-built partials (rule of janus_whisper_decode_beam_ex, 3 - 5): tokens
 * [rows][ld], done / sum_lp / n_tok / plen / row_rules per row, nlive / nfin / wdone / moved
 * per window, parent per row, fin_tok [windows][beam_size][ld], fin_s / fin_n
 * [windows][beam_size].
 *
 * janus_beam_reorder_f16: kc / vc [layers][n_windows * beam_size][n_ctx][d] fp16 — row i of
 * every window whose moved flag is set takes positions 0 .. pos of row parent[i] of the same
 * window, in place.
 */
int janus_beam_partial_blocks(int V, int K, int max_blocks);
/*
 * janus_logits_partial_f16: the vocabulary projection's partials alone, greedy (inv_temp 0) or
 * sampling (inv_temp = 1 / T > 0 with seeds [batch] device uint32 and the position pos):
 * K = 384 / 512 / 768 (64-row groups), 1024 (48-row groups) or 1280 (32-row groups); parts [batch][nblk] x 56 B as
 * above, nblk = janus_beam_partial_blocks(V, K, max_blocks). target: the token whose raw logit
 * t_v tracks (-1: none).
 */
int janus_logits_partial_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                             int eot, int suppress_blank, int blank, int ts_begin,
                             int no_timestamps, int max_initial_ts, int target,
                             const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                             float inv_temp, const uint32_t* seeds, int pos, void* parts,
                             void* stream);
/*
 * History rules (janus_decode_options.repetition_penalty / no_repeat_ngram_size), the two kernels
 * alone. The history words: uint32 [groups][(V + 15) / 16 tiles][rg rows], rg = 64 rows per
 * group up to K = 768, 48 at K = 1024 and 32 at K = 1280, row b in group b / rg; bits 0-15 of a word are the
 * tile's penalised columns, bits 16-31 its banned ones. janus_history_words returns their
 * count for batch rows (a count, not a status).
 *
 * janus_history_rules: positions pos0 .. pos0 + n_pos - 1 of every row in turn, one launch
 * each, as a decode call's positions run it: tokens [batch][ld] int32 (given rows, nothing is
 * sampled), plen [batch] the rows' prompt lengths, n = no_repeat_ngram_size, hist the words
 * (the caller zeroes them before a row's first position).
 *
 * janus_logits_partial_hist_f16: janus_logits_partial_f16 with the history words applied in
 * the epilogue (hist as above for this K, repetition_penalty > 0): the penalised, banned
 * logits go through the filter, t_v / m_raw / s_raw stay on the raw ones.
 */
int janus_history_words(int V, int K, int batch);
int janus_history_rules(const int32_t* tokens, int ld, int batch, const int32_t* plen, int n, int V,
                        int K, int pos0, int n_pos, uint32_t* hist, void* stream);
int janus_logits_partial_hist_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                                  int eot, int suppress_blank, int blank, int ts_begin,
                                  int no_timestamps, int max_initial_ts, int target,
                                  const uint8_t* smask, const int32_t* row_rules, int max_blocks,
                                  float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                  const uint32_t* hist, float repetition_penalty, void* stream);
/* Int8 decoder weights (rule at janus_whisper_set_decoder_compute, janus.h).
 * janus_quant_weight_rows_i8: x fp16 [M][K] (row stride ldx) -> q int8 [M][K] (row stride
 * ldq), scale [M]; any K % 8 == 0.
 * janus_gemm_w8_f16: janus_gemm_f16 with W replaced by q int8 [N][K] (row stride ldw) and
 * scale [N]; M <= 512 rows on the skinny kernel, epi also 4 (the QKV cache epilogue is not
 * reachable here: 0 .. 3); a_group_cols > 0: the grouped (block-diagonal) product.
 * janus_logits_partial_w8_f16 / janus_logits_partial_hist_w8_f16: janus_logits_partial_f16 /
 * janus_logits_partial_hist_f16 with W replaced by the int8 table q [V][K] and scale [V]. */
int janus_quant_weight_rows_i8(const uint16_t* x, int64_t ldx, int8_t* q, int64_t ldq, float* scale, int M,
                               int K, void* stream);
int janus_gemm_w8_f16(int epi, const uint16_t* A, int64_t lda, const int8_t* q, const float* scale,
                      int64_t ldw, const float* bias, void* C, int64_t ldc, const float* R, int64_t ldr,
                      int M, int N, int K, int a_group_cols, void* stream);
int janus_logits_partial_w8_f16(const uint16_t* A, const int8_t* q, const float* scale, int K, int V, int batch,
                                int eot, int suppress_blank, int blank, int ts_begin, int no_timestamps,
                                int max_initial_ts, int target, const uint8_t* smask, const int32_t* row_rules,
                                int max_blocks, float inv_temp, const uint32_t* seeds, int pos, void* parts,
                                void* stream);
int janus_logits_partial_hist_w8_f16(const uint16_t* A, const int8_t* q, const float* scale, int K, int V,
                                     int batch, int eot, int suppress_blank, int blank, int ts_begin,
                                     int no_timestamps, int max_initial_ts, int target, const uint8_t* smask,
                                     const int32_t* row_rules, int max_blocks, float inv_temp,
                                     const uint32_t* seeds, int pos, void* parts, const uint32_t* hist,
                                     float repetition_penalty, void* stream);
/* One quantised matrix of a prepared context, read back to the host: layer 0 .. dec_layers - 1
 * and which = JANUS_DEC_W_*, or layer -1 (which ignored): the vocabulary table. q_out [host]
 * int8 [N][K], s_out [host] float [N]. Prepares the int8 copies if the context has none. */
int janus_whisper_decoder_weight_i8(janus_whisper* w, int layer, int which, int8_t* q_out, float* s_out);
int janus_beam_logits_topk_f16(const uint16_t* A, const uint16_t* W, int K, int V, int batch,
                               int eot, int suppress_blank, int blank, int ts_begin,
                               int no_timestamps, int max_initial_ts, const uint8_t* smask,
                               const int32_t* row_rules, int max_blocks, void* parts, void* tops,
                               int n2k, float* all_v, int32_t* all_i, float* ts_v, int32_t* ts_i,
                               void* stream);
int janus_beam_step(const void* parts, const void* tops, int nblk, int eot, int suppress_blank,
                    int blank, int ts_begin, int no_timestamps, int max_initial_ts,
                    int32_t* row_rules, int32_t* tokens, int ld, int pos, int32_t* done,
                    float* sum_lp, int32_t* n_tok, const int32_t* plen, int beam_size,
                    int n_windows, int32_t* nlive, int32_t* nfin, int32_t* wdone, int32_t* moved,
                    int32_t* parent, int32_t* fin_tok, float* fin_s, int32_t* fin_n, void* stream);
int janus_beam_reorder_f16(uint16_t* kc, uint16_t* vc, int layers, int n_windows, int beam_size,
                           int n_ctx, int d, int pos, const int32_t* parent, const int32_t* moved,
                           void* stream);

/*
 * Test-only view of the decode planner (csrc/decode_plan.h): the plan a decode call with
 * these arguments gets on a lane of `cus` CUs, without an engine or a device. `resident`
 * answers whether the persistent segments' grid is co-resident (the library asks the
 * device's occupancy; the two-blocks-per-CU grid of JANUS_DEC_PATH_SEG_2CU, which asks it
 * too, is described as the one-block-per-CU grid); multi_lane: the call is one lane of
 * several. temperature > 0 samples, temperatures [host] float [batch] (nullable) are per-row
 * temperatures, beam_size > 0 is a beam search over rows laid out as
 * janus_whisper_decode_beam_ex builds them. stand [host] int32 [n_stand] / stand_maxlen
 * (nullable / 0): where the lane's row slots stand for a staggered call.
 * text [text_cap]: the plan as name=value lines (fields only the code around the positions
 * reads as call.name), then pairs= and groups= as comma-separated integers (pairs: b0, b1,
 * e per pair; groups: 8 per group), NUL-terminated. key [key_cap]: the plan's contribution
 * to the graph cache key, *n_key values. A call the planner rejects, or a buffer too small,
 * returns non-zero with janus_last_error.
 */
int janus_decode_plan_describe(const janus_whisper_config* cfg, const janus_decode_options* opt,
                               const janus_decode_rows* rows, int batch, int cus, int resident,
                               int multi_lane, float temperature, const float* temperatures,
                               int beam_size, const int32_t* stand, int n_stand, int stand_maxlen,
                               char* text, int text_cap, int64_t* key, int key_cap, int32_t* n_key);
/* The same with the context's cross-attention compute type (JANUS_CROSS_COMPUTE_*,
 * janus_whisper_set_cross_compute) as the call would find it; janus_decode_plan_describe is
 * this entry at JANUS_CROSS_COMPUTE_F16. */
int janus_decode_plan_describe_cross(const janus_whisper_config* cfg, const janus_decode_options* opt,
                                     const janus_decode_rows* rows, int batch, int cus, int resident,
                                     int multi_lane, float temperature, const float* temperatures,
                                     int beam_size, const int32_t* stand, int n_stand, int stand_maxlen,
                                     int cross_compute, char* text, int text_cap, int64_t* key,
                                     int key_cap, int32_t* n_key);
/* The same with the decoder weights' compute type as well (JANUS_DEC_COMPUTE_*,
 * janus_whisper_set_decoder_compute); janus_decode_plan_describe_cross is this entry at
 * JANUS_DEC_COMPUTE_F16. */
int janus_decode_plan_describe_modes(const janus_whisper_config* cfg, const janus_decode_options* opt,
                                     const janus_decode_rows* rows, int batch, int cus, int resident,
                                     int multi_lane, float temperature, const float* temperatures,
                                     int beam_size, const int32_t* stand, int n_stand, int stand_maxlen,
                                     int cross_compute, int dec_compute, char* text, int text_cap,
                                     int64_t* key, int key_cap, int32_t* n_key);

/*
 * Test-only view of the decoder's residual stream: a teacher-forced run of the decode call's
 * own machinery (plan, buffers, uploads, cross K/V, then every position's embedding and
 * layers with the plan's path flags and persistent level), launched directly, without the
 * final LayerNorm / vocabulary projection / selection. No sampling and no beam search: the
 * entry takes neither argument.
 *   rows      the forced tokens are the per-row prompts, every row the same length n (the
 *             entry runs with max_length = n + 1 whatever opt says); enc_index, pos_offset and
 *             steps as in janus_whisper_decode_greedy_ex, the continuation checks and the
 *             recorded stand (janus_whisper_decode_stand) included, so a second call with the
 *             same n continues rows. A continuing row's tokens are taken from its prompt too.
 *   x_out     [device] f32 [x_positions][batch][d_model]: row b of step i is the residual row
 *             (before the decoder's final LayerNorm) of position pos_offset[b] + i. The call
 *             runs steps positions (n when steps is 0 or the rows are not staggered) and
 *             fails when x_positions is smaller.
 *   kc_out / vc_out  [device, nullable] fp16 [dec_layers][batch][n_text_ctx][d_model]: the
 *             self-attention caches after the last position.
 *   plan_text [plan_cap]: the plan that ran, as janus_decode_plan_describe writes it.
 * Waits for the stream; a persistent segment's barrier timeout is an error, not data.
 */
int janus_whisper_decode_hidden(janus_whisper* w, const uint16_t* enc, int batch,
                                const janus_decode_options* opt, const janus_decode_rows* rows,
                                float* x_out, int x_positions, uint16_t* kc_out, uint16_t* vc_out,
                                char* plan_text, int plan_cap, void* stream);

/*
 * Word alignment kernels (janus_whisper_align), one test entry each. Device pointers.
 *
 * janus_align_dtw_f32: the DTW of janus.h's rule 4 on x f32 [N][F] as given (the alignment
 * call passes -A): cost[i][j] = x[i-1][j-1] + min(c0, c1, c2) with the comparisons in that
 * rule's order, so the path is exact for a given matrix, ties included. trace u8
 * [N + 1][F + 1] (scratch; the border entries are not written), text_indices / time_indices
 * int32 [N + F] (-1 past the path), path_len int32 [1]. N <= 511.
 *
 * janus_align_reduce_f32: probs f32 [heads][n][F] -> A f32 [n - sot_len - 1][F] (rule 3:
 * (P - mean) / std over the n rows per head and frame, median of 7 along the frames with
 * reflect padding unless F <= 3, mean over heads, rows sot_len .. n - 2).
 *
 * janus_align_token_prob_f16: prob[r] = softmax(LayerNorm(x[r]; gamma, beta, 1e-5) . W^T)
 * [target[r]] over the V columns of W fp16 [V][d] (rule 5 with V = eot); x f32 [rows][d],
 * target int32 [rows] in [0, V). The logits exist for one chunk of rows at a time.
 * Each of the three waits for the stream before it returns.
 */
int janus_align_dtw_f32(const float* x, int N, int F, uint8_t* trace, int32_t* text_indices,
                        int32_t* time_indices, int32_t* path_len, void* stream);
int janus_align_reduce_f32(const float* probs, int heads, int n, int F, int sot_len, float* A,
                           void* stream);
int janus_align_token_prob_f16(const float* x, const float* gamma, const float* beta,
                               const uint16_t* W, int rows, int d, int V, const int32_t* target,
                               float* prob, void* stream);

/*
 * The language head of janus_whisper_detect_language (langid.hip), one block per row:
 * probs[r] = softmax over l < n_lang of LayerNorm(x[r]; gamma, beta, 1e-5) . emb[lang_begin + l]
 * in fp32, best[r] = its argmax (lowest index on ties). x f32 [rows][d], emb fp16 with at
 * least lang_begin + n_lang rows of d, probs f32 [rows][n_lang], best int32 [rows]; device
 * pointers. 1 <= n_lang <= 128, d % 8 == 0, d <= 2048.
 */
int janus_lang_head_f16(const float* x, const float* gamma, const float* beta, const uint16_t* emb,
                        int d, int lang_begin, int n_lang, int rows, float* probs, int32_t* best,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JANUS_KERNELS_H_ */

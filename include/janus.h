/*
 * janus.h — C-ABI of libjanus_hip.so, the MI355X-native (gfx950) hot path of Janus.
 *
 * Every entry point returns int (0 = OK, non-zero = error; message from
 * janus_last_error(), per calling thread). No C++ exception crosses this ABI.
 * Arrays marked [device] are HIP device pointers the caller owns (e.g. torch
 * tensors); [host] arrays are ordinary memory. `stream` is a hipStream_t (NULL =
 * the null stream). Kernels are enqueued asynchronously on `stream`; host-side
 * entry points (packet codec) are synchronous and thread-safe.
 *
 * Each declaration names the reference interface it replaces (path:line in
 * akshatvasisht/janus). Reference bindings a maintainer would add: INTEGRATION.md.
 */
#ifndef JANUS_H_
#define JANUS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ errors */
const char* janus_last_error(void);
/* ABI version: major*10000 + minor*100 + patch. */
int janus_version(void);

/*
 * A HIP stream whose kernels run only on the CUs set in cu_mask (words x 32 bits, bit i =
 * CU i; hipExtStreamCreateWithCUMask). The pipeline runs the vocoder of one batch and
 * the latency-bound greedy decoder of the next on disjoint CU sets. Destroy with
 * janus_stream_destroy.
 */
int janus_stream_create_cu_mask(const uint32_t* cu_mask, int words, void** stream_out);
int janus_stream_destroy(void* stream);

/* ------------------------------------------------------------- prosody --- */
/*
 * Batched ProsodyExtractor core: aubio YIN per hop + RMS per utterance.
 * Replaces aubio.pitch('yin', 4096, hop, sr) with unit Hz / tolerance `tolerance`
 * (backend/services/prosody.py:32-34) called once per hop (prosody.py:78-87), and
 * numpy's rms = sqrt(mean(x**2)) (prosody.py:67). One stream per utterance:
 *   pcm            [device] f32, utterances back to back
 *   sample_offsets [device] int64[B+1], prefix offsets into pcm
 *   hop_offsets    [device] int64[B+1], prefix sum of ceil(n_b / hop)
 *   total_hops     host copy of hop_offsets[B]
 *   silence_db     aubio pitch silence threshold (aubio default -50 dB)
 *   state_in       [device] f32[B][4096] detector buffer before the call, or NULL (zeros)
 *   state_out      [device] f32[B][4096] buffer after the call, or NULL; must not alias state_in
 *   f0_out         [device] f32[total_hops] per-hop pitch in Hz (0 = unvoiced/silent)
 *   rms_out, mean_f0_out [device] f32[B]; n_voiced_out [device] int32[B]
 * rms_out is NaN for an empty utterance (numpy mean of an empty array).
 */
int janus_prosody_analyze(const float* pcm, const int64_t* sample_offsets,
                          const int64_t* hop_offsets, int batch, int64_t total_hops,
                          int sample_rate, int hop_size, float tolerance, float silence_db,
                          const float* state_in, float* state_out, float* f0_out,
                          float* rms_out, float* mean_f0_out, int32_t* n_voiced_out,
                          void* stream);
/*
 * Same, with the YIN grid capped at max_blocks workgroups (0 = one per hop): a batch run
 * beside other latency-bound work (the greedy decoder) leaves that work CUs to dispatch
 * onto. Results are identical for every max_blocks.
 */
int janus_prosody_analyze_ex(const float* pcm, const int64_t* sample_offsets,
                             const int64_t* hop_offsets, int batch, int64_t total_hops,
                             int sample_rate, int hop_size, float tolerance, float silence_db,
                             const float* state_in, float* state_out, float* f0_out,
                             float* rms_out, float* mean_f0_out, int32_t* n_voiced_out,
                             int max_blocks, void* stream);

/* ------------------------------------------------- receiver / streaming --- */
/*
 * Playback ducking, in place on int16 PCM [device] (n samples): replaces
 * apply_ducking_if_needed (backend/services/engine.py:94-134) for level in [0, 1):
 * s = int16(trunc(clip(float32(s) * level, -32768, 32767))), numpy's
 * np.clip(s.astype(np.float32) * level, -32768, 32767).astype(np.int16) bit for bit.
 * (level >= 1 and ducking-off / not-talking are pass-throughs the caller skips.)
 */
int janus_duck_pcm16(int16_t* pcm, int64_t n, float level, void* stream);

/*
 * Speech-gate probability per chunk: pcm [device] f32 [n_chunks][chunk_len] (e.g. the
 * 1536-sample 48 kHz capture chunks, audio_io.py:28-31), prob_out [device] f32[n_chunks].
 * Stands in for VoiceActivityDetector.is_speech (backend/services/vad.py:40-77: x[::3]
 * -> silero -> prob > threshold), whose weights are a remote torch.hub download:
 * prob = sigmoid((10 log10(mean(x[::decim]^2)) - center_db) / width_db).
 */
int janus_vad_energy(const float* pcm, int64_t n_chunks, int chunk_len, int decim,
                     float center_db, float width_db, float* prob_out, void* stream);

/*
 * The neural gate itself: VoiceActivityDetector.is_speech's model(chunk[::3], 16000)
 * (backend/services/vad.py:40-77; silero-vad v5, 16 kHz graph: 64-sample context + STFT
 * 256/128 + 4 conv blocks + LSTMCell(128) + sigmoid), from local weights. A context
 * holds the parameters by their silero state-dict names ("_model.stft.forward_basis_buffer",
 * "_model.encoder.{0..3}.reparam_conv.{weight,bias}", "_model.decoder.rnn.{weight_ih,
 * weight_hh,bias_ih,bias_hh}", "_model.decoder.decoder.2.{weight,bias}").
 * janus_vad_run: pcm [device] f32 [n_streams][n_chunks][chunk_len] (chunk[::decim] must
 * give 512 samples: 1536 / 3 for the 48 kHz capture chunks); the model state of each
 * channel, carried across calls as silero's stateful model object carries it
 * (the reference never resets it, vad.py:79-88): ctx_state [device] f32 [n_streams][64],
 * hc_state [device] f32 [n_streams][2][128] (zeros = fresh), updated in place;
 * prob_out [device] f32 [n_streams][n_chunks], channels in parallel, chunks in order.
 */
typedef struct janus_vad janus_vad;
int janus_vad_create(janus_vad** out);
int janus_vad_destroy(janus_vad* v);
int janus_vad_set_tensor(janus_vad* v, const char* name, const float* host, int64_t numel);
int janus_vad_run(janus_vad* v, const float* pcm, int n_streams, int n_chunks, int chunk_len,
                  int decim, float* ctx_state, float* hc_state, float* prob_out, void* stream);

/*
 * The same network over whole files (faster-whisper's vad_filter; vad_file.hip): pcm
 * [device] f32 = the 16 kHz audio of n_streams utterances concatenated, offsets [host]
 * [n_streams + 1] in samples. Stream s of L_s samples has n_s = L_s / 512 + 1 chunks
 * (faster-whisper's pad(audio, (0, 512 - len % 512)): a length that is a multiple of 512,
 * 0 included, gets one whole zero chunk); a sample index >= L_s reads as 0. Every stream
 * starts from zero state (context 0, h = c = 0: a fresh model per file), and the context of
 * chunk j is samples [512 j - 64, 512 j) of the SAME stream. prob [device] f32 [sum n_s],
 * stream-major. n_streams = 0 is a no-op. Everything up to the input half of the LSTM gates
 * runs batched over all chunks, then one sequential scan per stream, in passes of at most
 * max_chunks_per_pass chunks per stream (2 KB of context-owned workspace per chunk and
 * stream; results do not depend on it). 0 = the default: 16384 / n_streams chunks, rounded
 * down to a multiple of 16 and at least 16, i.e. 32 MB of workspace up to 1024 streams.
 *
 * Speech timestamps (services/vad_filter.py, faster-whisper's get_speech_timestamps;
 * parity unpinned against the package), w = 512, samples at 16 kHz:
 *   min_speech = 16 min_speech_duration_ms, pad = 16 speech_pad_ms, min_sil = 16
 *   min_silence_duration_ms, max_speech = 16000 max_speech_duration_s - w - 2 pad,
 *   min_sil_at_max = 1568, neg_threshold = max(threshold - 0.15, 0.01) unless given.
 *   State: triggered = false, temp_end = prev_end = next_start = 0. For window i, p:
 *   1. p >= threshold and temp_end: temp_end = 0; if next_start < prev_end: next_start = w i.
 *   2. p >= threshold and not triggered: triggered, start = w i; next window.
 *   3. triggered and w i - start > max_speech: with prev_end set, close at prev_end, then
 *      untrigger if next_start < prev_end, else open a speech at next_start; zero prev_end,
 *      next_start, temp_end. Without it, close at w i, zero the three, untrigger; next window.
 *   4. p < neg_threshold and triggered: temp_end = w i if unset; if w i - temp_end >
 *      min_sil_at_max: prev_end = temp_end; if w i - temp_end < min_sil: next window; else
 *      close at temp_end (kept only if end - start > min_speech), zero the three, untrigger.
 *   An open speech with n_samples - start > min_speech closes at n_samples. Padding: first
 *   start = max(0, start - pad); between neighbours with sil = next.start - end: sil < 2 pad
 *   splits it in the middle (end += sil / 2, next.start -= sil / 2), else both move by pad
 *   (clamped to [0, n_samples]); last end = min(n_samples, end + pad).
 */
int janus_vad_probs(janus_vad* v, const float* pcm, const int64_t* offsets, int n_streams,
                    int max_chunks_per_pass, float* prob, void* stream);

/* ---------------------------------------------------------- resampling --- */
/*
 * Band-limited resampling of f32 audio from sr_in to sr_out (resample.hip): the step
 * faster-whisper's decode_audio takes through PyAV / libswresample before the model sees a
 * file. That filter cannot be pinned offline (parity unpinned against PyAV / libswresample),
 * so the rule is stated here and tests/resample_ref.py evaluates it in float64.
 *
 * g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g.
 *   Filter: s = min(1, L / M), Z = 32, beta = 10, W = Z / s (half width in input samples),
 *     phi(u) = s sinc(s u) I0(beta sqrt(1 - (u / W)^2)) / I0(beta) for |u| < W, else 0,
 *     sinc(v) = sin(pi v) / (pi v).
 *   Output length: n_out = ceil(n_in L / M).
 *   Output n: p = n mod L, i = n div L, c = (p M) div L, frac = (p M mod L) / L;
 *     taps h_p[k] = phi(frac - k) over the integers k with |frac - k| < W, normalised in
 *     float64 so that sum_k h_p[k] = 1 and then rounded once to float32;
 *     y[n] = sum_k h_p[k] x[i M + c + k], x = 0 outside [0, n_in).
 *   Output n sits at input time n M / L: no delay, each phase's taps symmetric about it.
 * The kernel sums each output as one k-ordered fmaf chain in float32.
 *
 * Limits: both rates in 4000 .. 384000 and L <= 640 (44101 -> 16000 is refused); the message
 * names both rates. sr_in == sr_out is a copy (L = M = T = 1, the tap 1).
 *
 * janus_resample_plan: the host plan alone, no device. L, M, T (taps of the widest phase)
 * and, where the pointers are given, first [L] (output i L + p starts at x[i M + first[p]],
 * first[p] = c + the least k) and taps f32 [L][T] (phase p's row, zero past its last tap);
 * the capacities are in elements and are checked.
 *
 * A resampler holds the plan of one pair, its tap matrix on the device and a grow-only
 * staging buffer. janus_resampler_info: L, M, T, out_tile (the output samples one block of
 * the kernel computes for a clip) and front (the zeros the staging buffer holds in front of
 * each clip, >= ceil(W) + 1); any pointer may be null.
 *
 * janus_resample_f32: pcm [device] f32 = n_clips clips of rate sr_in concatenated, offsets
 * [host] [n_clips + 1] in samples, as janus_vad_probs takes them; out [device] f32,
 * out_offsets [host] [n_clips + 1] with out_offsets[c + 1] - out_offsets[c] = ceil(n_c L / M)
 * (checked). Clip c is copied behind `front` zeros into the staging buffer, zeros follow up
 * to the end of its last tile, and the kernel reads nothing else: no sample of one clip
 * reaches another clip's output and a clip's bits do not depend on what it is batched with.
 * n_clips = 0, or clips that are all empty, launch nothing.
 */
typedef struct janus_resampler janus_resampler;
int janus_resample_plan(int sr_in, int sr_out, int* L, int* M, int* T, int32_t* first,
                        int64_t first_capacity, float* taps, int64_t taps_capacity);
int janus_resampler_create(int sr_in, int sr_out, janus_resampler** out);
int janus_resampler_destroy(janus_resampler* r);
int janus_resampler_info(const janus_resampler* r, int* L, int* M, int* T, int* out_tile, int* front);
int janus_resample_f32(janus_resampler* r, const float* pcm, const int64_t* offsets, int n_clips,
                       float* out, const int64_t* out_offsets, void* stream);

/* -------------------------------------------------------- packet codec --- */
enum {
  JANUS_VAL_NIL = 0,
  JANUS_VAL_BOOL = 1,
  JANUS_VAL_INT = 2,   /* signed 64-bit in .i */
  JANUS_VAL_UINT = 3,  /* unsigned 64-bit in .i (bit pattern), > INT64_MAX only */
  JANUS_VAL_FLOAT = 4, /* float64 in .f */
  JANUS_VAL_STR = 5,   /* UTF-8 bytes: .s/.len (pack) or .offset/.len into the buffer (unpack) */
  JANUS_VAL_BIN = 6,
  JANUS_VAL_ARRAY = 7, /* .len children follow (pre-order) */
  JANUS_VAL_MAP = 8    /* .len key/value pairs follow (pre-order) */
};

typedef struct {
  int32_t type;
  int64_t i;
  double f;
  const char* s;
  size_t len;
} janus_value;

typedef struct {
  const char* text; /* UTF-8 */
  size_t text_len;
  int64_t mode; /* int(JanusMode) */
  int32_t n_prosody;
  const janus_value* prosody_keys; /* JANUS_VAL_STR, in dict insertion order */
  const janus_value* prosody_vals;
  const char* override_emotion; /* NULL => key 'o' omitted (override == "Auto") */
  size_t override_len;
  janus_value timestamp; /* JANUS_VAL_FLOAT (time.time()) or JANUS_VAL_INT */
} janus_packet;

/*
 * Replaces msgpack.packb(JanusPacket.to_dict(), use_bin_type=True)
 * (backend/common/protocol.py:57-76, :97-107). Keys in insertion order t, m, p, ts[, o].
 * Writes up to `cap` bytes; *out_len is the full size (error if it exceeds cap).
 */
int janus_pack_packet(const janus_packet* pkt, uint8_t* out, size_t cap, size_t* out_len);

typedef struct {
  int32_t type;  /* JANUS_VAL_* */
  int64_t i;     /* INT/UINT/BOOL value */
  double f;      /* FLOAT value */
  size_t offset; /* STR/BIN: byte offset of the payload in the input buffer */
  size_t len;    /* STR/BIN: payload bytes; ARRAY: items; MAP: pairs */
} janus_mp_node;

/*
 * Replaces msgpack.unpackb(payload, raw=False) (backend/common/protocol.py:109-121).
 * Decodes one MessagePack object into `nodes` (pre-order); fails on truncated input,
 * trailing bytes (msgpack ExtraData), the reserved byte 0xc1 and ext types.
 */
int janus_unpack(const uint8_t* buf, size_t len, janus_mp_node* nodes, size_t cap,
                 size_t* n_nodes);


/* ------------------------------------------------------------ whisper --- */
/*
 * Whisper speech-to-text on the GPU. Replaces faster-whisper's WhisperModel
 * (CTranslate2) as constructed at backend/services/transcriber.py:23-27 and driven by
 * model.transcribe(audio[::3], beam_size=1, language='en') at :51-57 (one 30 s window
 * per utterance). fp16 tensors are passed as uint16_t (IEEE binary16 bits).
 */
typedef struct {
  int n_mels;      /* 80; 128 for the large-v3 family (no other value is accepted) */
  int n_audio_ctx; /* 1500 encoder positions (3000 mel frames) */
  int d_model;     /* 384 tiny, 512 base, 768 small, 1024 medium.en / distil-medium.en, 1280 large-v3 /
                      large-v3-turbo / distil-large-v3 */
  int n_heads;     /* d_model / 64: up to 20. At 1024 / 16 and 1280 / 20 heads the decode call runs the launch
                      path (persistent > 0 reports level 0), rows sharing an encoder row are gathered, every
                      d_model <= 512 fusion is off, and beam search (janus_whisper_decode_beam_ex) and the
                      int8 encoder are refused (non-zero status); janus_whisper_align runs up to d_model 1024
                      and is refused at 1280. Its default alignment set (every head of the last half of the
                      decoder layers) must not exceed 64 heads: medium.en's 192 are refused (non-zero status)
                      until janus_whisper_set_alignment_heads names at most 64 */
  int enc_layers;
  int dec_layers;
  int n_vocab;     /* 51864 for *.en, 51865 multilingual, 51866 the large-v3 family (100 languages) */
  int n_text_ctx;  /* 448 */
} janus_whisper_config;

typedef struct janus_whisper janus_whisper;

int janus_whisper_create(const janus_whisper_config* cfg, janus_whisper** out);
int janus_whisper_destroy(janus_whisper* w);
/*
 * Upload one fp32 parameter [host] by its Hugging Face Whisper name without the
 * "model." prefix (e.g. "encoder.layers.0.fc1.weight"), plus the two front-end
 * constants "mel.basis" [400][416] (periodic-Hann-weighted cos|sin DFT basis, 208
 * bins each) and "mel.filters" [208][n_mels] (slaney mel filters, transposed, zero-padded).
 */
int janus_whisper_set_tensor(janus_whisper* w, const char* name, const float* host,
                             int64_t numel);
/*
 * Log-mel features (faster-whisper FeatureExtractor, n_fft 400, hop 160, n_mels = 80 or 128
 * mels, 3000 frames) of x[::decim] for each utterance of pcm [device] (offsets [device]
 * int64[B+1]). logmel [device] f32 [B][3000][n_mels] (raw log10 mel, may be NULL), mel
 * [device] fp16 [B][3000][n_mels] (clamped and scaled). The first 30 s window of each clip as
 * faster-whisper's generate_segments feeds it to the encoder: frames from len(x16) // 160
 * on are 0.0 (pad_or_trim of the content frames), the global max is over the frames that
 * reach the first 30 s + 2 frames of audio (the whole clip when it is <= 30 s).
 */
int janus_whisper_logmel(janus_whisper* w, const float* pcm, const int64_t* offsets, int batch,
                         int decim, float* logmel, uint16_t* mel, void* stream);
/*
 * The whole-clip log-mel faster-whisper computes once per transcribe() call
 * (transcriber.py:53-57 -> WhisperModel.transcribe -> FeatureExtractor(audio)): `frames`
 * frames per utterance, mel [device] fp16 [B][frames][n_mels], normalised with the maximum over
 * every frame of the clip, frames from len(x16) // 160 on 0.0. Its 30 s windows are the
 * slices [seek, seek + min(3000, content - seek)) padded with zeros to 3000 frames.
 */
int janus_whisper_logmel_frames(janus_whisper* w, const float* pcm, const int64_t* offsets,
                                int batch, int decim, int frames, uint16_t* mel, void* stream);
/* Encoder forward: mel [device] fp16 [B][3000][n_mels] -> enc [device] fp16 [B][1500][d]. */
int janus_whisper_encode(janus_whisper* w, const uint16_t* mel, int batch, uint16_t* enc,
                         void* stream);
/*
 * Compute type of the encoder's linear layers (fused QKV, out_proj, fc1, fc2 of every
 * encoder layer). F16 (the default): fp16 weights and activations on the fp16 MFMA. INT8:
 * CTranslate2's int8 compute type (transcriber.py:23-27, compute_type='int8') — weights
 * quantised per output row from the fp32 parameters on first use (and again after a
 * janus_whisper_set_tensor), activations per row on the fly, int32 accumulation on the i8
 * MFMA. The conv stem, attention, LayerNorms, residual stream and the whole decoder are the
 * same in both modes (the decoder's weights have a switch of their own,
 * janus_whisper_set_decoder_compute). The mode may be switched between calls, in either direction.
 */
#define JANUS_ENC_COMPUTE_F16 0
#define JANUS_ENC_COMPUTE_INT8 1
int janus_whisper_set_encoder_compute(janus_whisper* w, int mode);
int janus_whisper_encoder_compute(janus_whisper* w, int32_t* mode);
/*
 * Compute type of the decoder's cross-attention operand: the encoder output E the decode
 * calls are handed. F16 (the default): the cross-attention streams E as given. INT8:
 * CTranslate2's int8 compute type quantises the input of the cross-attention K / V
 * projections row by row; here those projections are absorbed into the query, so the same
 * quantisation lands on E itself:
 *  1. Every decode call quantises its encoder rows E [n][Te][d] (fp16) once, before its first
 *     position, per key row t with the int8 encoder's rule: amax = max_j |E[t][j]|,
 *     q[t][j] = clamp(rint(E[t][j] * (127 / amax)), -127, 127), s[t] = amax / 127; a zero row
 *     gives q = 0, s = 1.
 *  2. The cross-attention of every layer, row and position sees
 *     E'[t][j] = fp16_rn(float(q[t][j]) * s[t]) in place of E[t][j]: the product taken in fp32
 *     and rounded once to fp16 (numpy: (q.astype(float32) * s[:, None]).astype(float16)). It
 *     streams q (1 byte per element) and s (4 bytes per key) instead of E (2 bytes).
 *  3. Everything after that is the fp16 call's arithmetic: scores, softmax, context rows,
 *     value and output projections.
 * Honoured by janus_whisper_decode_greedy(_ex), _sample_ex, _sample_rows_ex and _beam_ex (and
 * the test entry janus_whisper_decode_hidden), shared encoder rows (enc_index: rows read in
 * place are quantised where they lie, gathered rows gather q and s) and staggered rows (a
 * continuing call quantises the rows it is handed again) included. A `persistent` request runs
 * the launch path (janus_whisper_decode_path reports 0), as beam search does.
 * JANUS_DEC_PATH_NO_XABSORB, JANUS_DEC_PATH_XGROUP and JANUS_DEC_PATH_XROWS(n) with INT8 are
 * REJECTED (non-zero status, janus_last_error, nothing enqueued), as is a call of more than
 * 512 rows. janus_whisper_align and janus_whisper_detect_language keep reading the fp16 E
 * whatever the mode. The mode may be switched between calls, in either direction; F16 again
 * is bit-identical to a context that never left it. janus_whisper_decode_cross tells which
 * operand the last decode call read.
 */
#define JANUS_CROSS_COMPUTE_F16 0
#define JANUS_CROSS_COMPUTE_INT8 1
int janus_whisper_set_cross_compute(janus_whisper* w, int mode);
int janus_whisper_cross_compute(janus_whisper* w, int32_t* mode);
/* The JANUS_CROSS_COMPUTE_* the last decode call on this context ran with (the lane
 * janus_whisper_decode_path reports; JANUS_CROSS_COMPUTE_F16 before any call). */
int janus_whisper_decode_cross(janus_whisper* w, int32_t* mode);
/*
 * Compute type of the decoder's weights. F16 (the default): every decoder linear layer and
 * the vocabulary projection multiply the prepared fp16 weights. INT8: W8A16, weights int8,
 * activations fp16 as in F16.
 *  1. Quantisation. Per output row n of each prepared fp16 weight matrix W16 [N][K] (the fp16
 *     copy the F16 path multiplies): amax = max_k |W16[n][k]|,
 *     q[n][k] = clamp(rint(float(W16[n][k]) * (127 / amax)), -127, 127), s[n] = amax / 127; a
 *     zero row gives q = 0, s = 1. float32 arithmetic with IEEE division (no reciprocal
 *     approximation): numpy float32 reproduces q and s exactly; the rule of
 *     janus_whisper_set_cross_compute. Matrices, per decoder layer (JANUS_DEC_W_*): the fused
 *     self-attention QKV weight, the self-attention output projection, the absorbed
 *     cross-attention query weight (quantised from its fp16 absorbed form), the cross-attention
 *     value and output projections, fc1, fc2; and the token embedding as the vocabulary
 *     projection's table. The copies are made on the first decode call in the mode and again
 *     after janus_whisper_set_tensor.
 *  2. Product. A layer output is y[m][n] = s[n] * sum_k a[m][k] * q[n][k] + bias[n]: a fp16, q
 *     converted exactly to fp16, the products on the fp16 MFMA with fp32 accumulation, scale
 *     and bias applied in fp32, then the F16 path's epilogue (fp16 store, GELU, the QKV cache
 *     write, the fp32 residual add). A logit is s[v] * sum_k a[k] * q[v][k]; the rule filter,
 *     statistics, Gumbel keys and history rules run on it unchanged.
 *  3. Unchanged whatever the mode: the embedding lookup (it reads the fp16 table), the
 *     LayerNorms, both attentions, the residual stream, janus_whisper_align,
 *     janus_whisper_detect_language and the encoder. The fp16 weights stay resident: the int8
 *     copies are extra memory, not a saving.
 * Under INT8 every layer runs unfused (a LayerNorm launch in front of each projection, the
 * cross-attention's split merge and the value projection as two launches) and a `persistent`
 * request runs the launch path (janus_whisper_decode_path reports 0). Honoured by
 * janus_whisper_decode_greedy(_ex), _sample_ex, _sample_rows_ex and the test entry
 * janus_whisper_decode_hidden, shared encoder rows, staggered rows and the history rules
 * included, and composed with JANUS_CROSS_COMPUTE_INT8. REJECTED with INT8 (non-zero status,
 * janus_last_error, nothing enqueued): janus_whisper_decode_beam_ex, JANUS_DEC_PATH_NO_XABSORB,
 * JANUS_DEC_PATH_XGROUP and a call of more than 512 rows. The mode may be switched between
 * calls, in either direction; F16 again is bit-identical to a context that never left it.
 * janus_whisper_decode_weights tells which weights the last decode call multiplied.
 */
#define JANUS_DEC_COMPUTE_F16 0
#define JANUS_DEC_COMPUTE_INT8 1
int janus_whisper_set_decoder_compute(janus_whisper* w, int mode);
int janus_whisper_decoder_compute(janus_whisper* w, int32_t* mode);
/* The JANUS_DEC_COMPUTE_* the last decode call on this context ran with (the lane
 * janus_whisper_decode_path reports; JANUS_DEC_COMPUTE_F16 before any call). */
int janus_whisper_decode_weights(janus_whisper* w, int32_t* mode);
/* the quantised matrices of a decoder layer (janus_whisper_decoder_weight_i8, janus_kernels.h) */
#define JANUS_DEC_W_QKV 0     /* [3 d][d] */
#define JANUS_DEC_W_O 1       /* [d][d] */
#define JANUS_DEC_W_XQK 2     /* [H d][d], the absorbed cross-attention query weight */
#define JANUS_DEC_W_XV 3      /* [d][d] */
#define JANUS_DEC_W_XO 4      /* [d][d] */
#define JANUS_DEC_W_FC1 5     /* [4 d][d] */
#define JANUS_DEC_W_FC2 6     /* [d][4 d] */

typedef struct {
  const int32_t* prompt;   /* [host] initial tokens, e.g. {<|startoftranscript|>} for *.en */
  int prompt_len;
  int max_length;          /* total tokens incl. prompt (faster-whisper max_length 448) */
  int eot;
  const int32_t* suppress; /* [host] always-suppressed token ids (suppress_tokens=[-1] set) */
  int n_suppress;
  int suppress_blank;      /* SuppressBlank at the first sampled token */
  int blank_token;         /* " " token id */
  int timestamp_begin;     /* first timestamp token id, -1 = no timestamp rules */
  int no_timestamps;       /* <|notimestamps|> id */
  int max_initial_timestamp_index; /* 50 (= 1.0 s), -1 = unbounded */
  int check_every;         /* poll for all-rows-finished every N steps (0 = never) */
  int xattn_splits;        /* cross-attention key splits per utterance (0 = auto: 8; the
                              overlapped step on half the CUs runs best at 4) */
  int cu_count;            /* CUs the decoder's stream may use (0 = the popcount of the
                              stream's CU mask), e.g. 128 on a half-GPU partition: one
                              vocabulary-projection block per CU, and at <= 128 the skinny
                              projections split rows from N <= 1024 */
  int state_slot;          /* decoder state slot of the context (0 = default): the KV caches,
                              tokens and rule state a call leaves behind for staggered
                              continuation live in this slot, so a sampled re-decode between
                              two staggered calls runs in another slot without disturbing
                              them (0 .. 7) */
  int logits_blocks;       /* vocabulary-projection blocks (0 = cu_count) */
  int msplit_rows_n;       /* skinny projections split rows over blocks up to this N
                              (0 = auto: 1024 on <= 128 CUs, else none; -1 = never) */
  int persistent;          /* 1: the launches between a layer's self- and cross-attention
                              run as two resident-grid launches with in-launch barriers
                              (d_model 512, 8 heads, <= 256 rows, >= 16 CUs per 16 rows up to
                              128 rows, 128 CUs at 256 rows; the other shapes keep the launch
                              path): 29 launches per position
                              at base.en instead of 75. Same arithmetic per row except the
                              GEMMs' k order (fp32-rounding level, not bit-identical to 0).
                              2: one launch per layer step — segment B of layer l, the
                              self-attention of l + 1 (one wave per row and head, online
                              softmax over 64-key chunks) and segment A of l + 1 as one
                              grid (layer 0's QKV, self-attention and segment A one head
                              grid, the final LayerNorm the last segment's phase): 16
                              launches per position (every row's keys in two
                              parts cut by its own length, merged in order: rows stay
                              independent of their neighbours).
                              3: as 2, with the cross-attention as the last phase of the
                              head / layer grids: 10 launches per position, measured level
                              with 2 */
  uint32_t path_flags;     /* alternative decoder paths (JANUS_DEC_PATH_* bits), for the
                              parity tests that hold every path bit-identical and for A/B
                              measurements; 0 = the measured default */
  int lanes;               /* concurrent decoder lanes of janus_whisper_decode_greedy: the
                              batch split over streams and host threads (0 = 1; slower at
                              B = 64) */
  /* History rules: repetition_penalty p (> 0; 0 and 1 = off, so zeroed fields are a call
   * without them) and no_repeat_ngram_size n (>= 0; 0 = off), faster-whisper's options of the
   * same names. CTranslate2 cannot be run offline, so this rule is PARITY UNPINNED (as the beam
   * search and alignment rules); what is built, per row, with g the tokens the row has SAMPLED
   * in this call (timestamps included; the prompt — <|startofprev|> text, hotwords, the sot
   * sequence — is not part of g) and m = len(g):
   *  1. Penalty: for every distinct token t of g, logit[t] = logit[t] * p if logit[t] < 0,
   *     else logit[t] / p. Once per distinct token, in fp32, before every other rule.
   *  2. No-repeat n-grams: the tokens { g[i+n-1] : 0 <= i <= m-n and g[i .. i+n-2] ==
   *     g[m-n+1 .. m-1] } are banned, i.e. treated exactly like the suppress list (-inf).
   *     n = 1 bans every token of g; nothing is banned while m < n; overlapping matches count.
   *  3. Everything after runs unchanged on the penalised, banned logits: SuppressBlank, the
   *     timestamp rules, the timestamp-mass rule, the filtered log-sum-exp, the argmax (or
   *     Gumbel-max with key = penalised logit * 1/T + noise) and the accumulated
   *     log-probability (untempered, penalised, filtered).
   *  4. The raw statistics behind no_speech_prob stay unpenalised.
   * Honoured by janus_whisper_decode_greedy_ex, _sample_ex and _sample_rows_ex, shared
   * encoder rows (enc_index) included, for one more small launch per position; REJECTED
   * (non-zero status, janus_last_error, nothing enqueued) with beam search, with staggered
   * rows (pos_offset), for p < 0 and for n < 0. A `persistent` request with history rules
   * runs the launch path (janus_whisper_decode_path reports 0). */
  float repetition_penalty;
  int no_repeat_ngram_size;
} janus_decode_options;

/* janus_decode_options.path_flags */
#define JANUS_DEC_PATH_NO_GRAPH     0x0001u /* launch every position, no captured graph */
#define JANUS_DEC_PATH_NO_XABSORB   0x0002u /* per-layer cross K/V instead of the absorbed
                                               cross-attention over the encoder output */
#define JANUS_DEC_PATH_NO_XPAIR     0x0004u /* rows sharing an encoder row: no PAIR blocks */
#define JANUS_DEC_PATH_XGROUP       0x0008u /* ... GROUP blocks of up to 6 rows */
#define JANUS_DEC_PATH_FUSED_LN     0x0010u /* LayerNorm statistics on the projections */
#define JANUS_DEC_PATH_LN_FUSE      0x0020u /* LayerNorm in the producing kernels */
#define JANUS_DEC_PATH_RESID_LN     0x0040u /* whole-row residual projection + LayerNorm */
#define JANUS_DEC_PATH_NO_CVP       0x0080u /* split merge and value projection apart */
#define JANUS_DEC_PATH_CVP          0x0100u /* ... fused, above 64 rows too */
#define JANUS_DEC_PATH_NO_SEL_EMBED 0x0200u /* token selection and embedding apart */
#define JANUS_DEC_PATH_NO_EMBED_LN  0x0400u /* first LayerNorm not in the embedding kernel */
#define JANUS_DEC_PATH_LN_PROLOGUE  0x0800u /* LayerNorm-into-prologue mask m (bits 12-15:
                                               1 LN1, 2 LN2, 4 LN3, 8 final) instead of the
                                               default 9 up to 64 rows, 0 above */
#define JANUS_DEC_PATH_LN_MASK(m)   (JANUS_DEC_PATH_LN_PROLOGUE | (((uint32_t)(m) & 15u) << 12))
#define JANUS_DEC_PATH_SEG_2CU      0x10000u /* persistent segments at 256 rows: two blocks
                                               per CU instead of one block per CU taking two
                                               blocks' work */
#define JANUS_DEC_PATH_XFWD         0x20000u /* persistent segments: every layer's one-split
                                               cross-attention over the key chunks first to
                                               last (default: odd layers last to first) */
#define JANUS_DEC_PATH_XROWS(n)     ((((uint32_t)(n) >> 1) & 3u) << 18)
                                            /* 12 heads, d_model 768: rows sharing an encoder
                                               row read it in place in blocks of up to n = 2
                                               or 4 rows (default: one gathered copy per row,
                                               measured faster at 320 rows) */

/*
 * Batched greedy decoding (temperature 0) with the Whisper logit rules
 * (SuppressBlank, SuppressTokens, ApplyTimestampRules), KV cache on the device.
 * tokens [device] int32 [B][max_length] (prompt, then sampled tokens; -1 past the
 * end), n_tokens [device] int32 [B] sampled tokens incl. <|endoftext|>,
 * sum_logprob [device] f32 [B] (sum of chosen-token log-probabilities).
 */
int janus_whisper_decode_greedy(janus_whisper* w, const uint16_t* enc, int batch,
                                const janus_decode_options* opt, int32_t* tokens,
                                int32_t* n_tokens, float* sum_logprob, void* stream);

/*
 * Per-row prompts and the no-speech probability (faster-whisper's generate_segments /
 * generate_with_fallback state, transcriber.py:53-57 with its defaults):
 *   prompts      [host] int32 [B][stride]: row b's prompt (e.g. <|startofprev|>, the
 *                previous window's last <= 223 tokens, <|startoftranscript|> — the
 *                condition_on_previous_text prompt), prompt_lens [host] int32 [B];
 *                NULL prompts = opt->prompt for every row
 *   no_speech_token  token whose raw (unfiltered) softmax probability at the row's first
 *                sampled step is reported (<|nocaptions|> 50361 for *.en), -1 = none
 */
typedef struct {
  const int32_t* prompts;
  const int32_t* prompt_lens;
  int stride;
  int no_speech_token;
  /* Shared encoder outputs (faster-whisper's best_of hypotheses of one window,
   * transcriber.py:53-57 with the library's defaults): enc_index [host] int32 [B], row b
   * attends to encoder row enc_index[b] of enc, which then holds n_enc rows [n_enc][Te][d]
   * instead of B. The cross-attention reads each shared row once per PAIR of decoder rows
   * (both rows' heads in one MFMA tile) up to 8 heads / d_model 512; the 12-head models
   * (d_model 768) gather one copy of its encoder row per decoder row unless
   * JANUS_DEC_PATH_XROWS(n) asks for in-place blocks of n rows; janus_whisper_decode_path
   * tells which of the two a call did. NULL = row b attends to enc row b. */
  const int32_t* enc_index;
  int n_enc;
  /* Staggered decode (continuous batching across calls): pos_offset [host] int32 [B], row b
   * runs positions [pos_offset[b], pos_offset[b] + steps) (steps 0 = max_length - 1). A row
   * with an offset > 0 CONTINUES the previous call's row in the same slot of this context
   * (its tokens, KV cache, counters and rule state are kept; pass its encoder output again);
   * rows with offset 0 start fresh and must be one contiguous range. A continuing row's
   * offset must not exceed the position its previous calls reached (its tokens and KV rows
   * below the offset must have been written): the context records where every slot stands
   * after each call (janus_whisper_decode_stand) and REJECTS (non-zero status,
   * janus_last_error) a continuing row past it, or a continuing call whose batch size /
   * max_length differ from the previous call's. When every row finishes early (check_every
   * polls), all rows stand at offset + the positions actually run. Greedy only, no
   * enc_index; steps >= 0; pos_offset + steps <= max_length. NULL = every row fresh. */
  const int32_t* pos_offset;
  int steps;
  /* Where no_speech_prob is read: row b's no_speech_prob is the raw softmax probability of
   * no_speech_token from the logits at position prompt_lens[b] - 1 - no_speech_back. 0 (the
   * *.en models, whose prompt ends in <|startoftranscript|>): the prompt's last position,
   * i.e. the first sampled step. The multilingual models' prompt ends in [sot, language,
   * task], so <|startoftranscript|> lies two positions earlier: no_speech_back 2. The
   * vocabulary projection then runs from the earliest such position on; the rows keep their
   * forced tokens there and no rule state, counter or token is touched. Applies to every
   * decode form (greedy, sampled, per-row temperatures, shared encoder rows, staggered
   * fresh rows, persistent, beam). Each row needs 0 <= no_speech_back < prompt_lens[b], else
   * the call is rejected (non-zero status, janus_last_error). */
  int no_speech_back;
} janus_decode_rows;

/*
 * janus_whisper_decode_greedy with per-row prompts (rows may be NULL): all rows step
 * together, a row samples from its own prompt length on; tokens [device] int32
 * [B][max_length] hold row b's prompt in [0, prompt_lens[b]) and its sampled tokens after.
 * no_speech_prob [device] f32 [B] (nullable).
 */
int janus_whisper_decode_greedy_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                   const janus_decode_options* opt, const janus_decode_rows* rows,
                                   int32_t* tokens, int32_t* n_tokens, float* sum_logprob,
                                   float* no_speech_prob, void* stream);

/*
 * janus_whisper_decode_greedy_ex at temperature > 0: faster-whisper's fallback re-decode
 * (generate_with_fallback, temperatures 0.2 ... 1.0 with best_of 5: CTranslate2
 * generate(sampling_temperature=T, sampling_topk=0, num_hypotheses=5); the caller
 * replicates a window's row per hypothesis). Every token is drawn from softmax(l / T)
 * over the rule-filtered logits l by Gumbel-max; the noise is a counter-based hash of
 * (seeds[b], position, token), seeds [host] uint32 [B], so a row's draws are independent
 * of its batch neighbours and reproducible on the CPU. sum_logprob accumulates the chosen
 * tokens' log-probabilities under the untempered filtered distribution (the scores
 * CTranslate2 gathers from its log-softmax). temperature <= 0 or null seeds: error.
 */
int janus_whisper_decode_sample_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                   const janus_decode_options* opt, const janus_decode_rows* rows,
                                   float temperature, const uint32_t* seeds, int32_t* tokens,
                                   int32_t* n_tokens, float* sum_logprob, float* no_speech_prob,
                                   void* stream);

/*
 * janus_whisper_decode_sample_ex with a temperature per row: temperatures [host] f32 [B],
 * each >= 0 (0: a greedy row, as janus_whisper_decode_greedy_ex; its seed is ignored).
 * Row b's tokens equal those of a greedy / decode_sample_ex call at temperatures[b] with
 * the same seed (rows are independent of their batch neighbours), so a window's T = 0 row
 * and the hypotheses of every fallback temperature can run in ONE call and the caller keeps
 * exactly what the sequential generate_with_fallback walk (transcriber.py:53-57,
 * faster-whisper's temperature loop) keeps: janus_amd/services/transcriber.py
 * generate_segments(speculative=True), the streaming encoder's setting.
 */
int janus_whisper_decode_sample_rows_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                        const janus_decode_options* opt, const janus_decode_rows* rows,
                                        const float* temperatures, const uint32_t* seeds,
                                        int32_t* tokens, int32_t* n_tokens, float* sum_logprob,
                                        float* no_speech_prob, void* stream);

/*
 * Beam search at temperature 0 (faster-whisper's beam_size, 1 .. 8; patience 1): enc
 * [n_windows][1500][d], rows->prompts / prompt_lens one prompt per WINDOW (null rows or null
 * prompts: opt->prompt for every window; rows->enc_index and pos_offset must be null, the
 * call builds the windows x beam_size decoder rows and their shared encoder rows itself).
 * Outputs one row per window: tokens [n_windows][max_length], n_tokens, sum_logprob,
 * no_speech_prob [n_windows]. n_windows * beam_size <= 512; a `persistent` request runs
 * the launch path. CTranslate2's beam search cannot be pinned offline; the rule built here,
 * per window with k = beam_size:
 *  1. Up to k live beams, each with its sampled tokens, cumulative score S (the sum of the
 *     untempered rule-filtered log-probs, as the greedy sum_logprob) and rule state; a list
 *     of at most k finished hypotheses. At the first sampled position only beam 0 is live.
 *  2. Every live beam's log-probs come from the decoding rules applied to its own tokens
 *     (suppress list, SuppressBlank, timestamp rules, max_initial_timestamp and the
 *     timestamp-mass rule, which renormalises over the timestamps).
 *  3. Candidates (S_b + lp_b[v], b, v) over live beams and allowed tokens: the best 2k,
 *     ordered by score descending, then smaller b, then smaller v.
 *  4. Walked in order: v == eot is appended to the finished list while it holds fewer than k,
 *     with normalised score S / n^length_penalty (n = sampled tokens incl. eot); any other
 *     candidate becomes the next live beam until k are filled, then the walk stops. A child
 *     inherits its parent's tokens, rule state and self-attention K / V rows.
 *  5. The window stops when its finished list holds k, or at max_length, where the live
 *     beams close as they stand with S / (n + 1)^length_penalty.
 *  6. The finished hypothesis with the highest normalised score wins (earliest on ties); if
 *     none finished, the best closed live beam. no_speech_prob is beam 0's first step's.
 * beam_size 1 is the greedy decode.
 */
int janus_whisper_decode_beam_ex(janus_whisper* w, const uint16_t* enc, int n_windows,
                                 const janus_decode_options* opt, const janus_decode_rows* rows,
                                 int beam_size, float length_penalty, int32_t* tokens,
                                 int32_t* n_tokens, float* sum_logprob, float* no_speech_prob,
                                 void* stream);

/*
 * Shape of the last decode call on this context (lane 0): positions the decoder stepped
 * (every row together; the early-exit poll stops at a 16-position boundary) and the
 * kernel launches those positions issued (nodes of the captured decode graphs; 0 when
 * JANUS_NO_GRAPH runs without graphs). Measurement only (bench.py's decoder roofline:
 * launches per position beside bytes per position); the reference has no counterpart.
 */
int janus_whisper_decode_info(janus_whisper* w, int32_t* positions, int64_t* launches);

/*
 * Which path the last decode call on this context took (the lane janus_whisper_decode_info
 * reports), read-only:
 *   enc_rows    how the decoder rows reached their encoder output: JANUS_ENC_ROWS_OWN (no
 *               enc_index: row b reads enc row b), JANUS_ENC_ROWS_IN_PLACE (enc_index: every
 *               shared encoder row read in place, once per block of decoder rows — PAIR blocks
 *               up to 8 heads; at 12 heads / d_model 768 blocks of two or four rows with
 *               JANUS_DEC_PATH_XROWS(n)) or
 *               JANUS_ENC_ROWS_GATHERED (enc_index: one copy of its encoder row per decoder
 *               row, [Te][d] fp16 each — JANUS_DEC_PATH_NO_XPAIR / _NO_XABSORB, the 12-head
 *               family's default, or a shape without a shared-row kernel)
 *   persistent  the persistent level the call actually ran (0: the launch path; 1..3 as
 *               janus_decode_options.persistent) — a shape the persistent segments do not
 *               cover (any d_model but 512) silently keeps the launch path and reports 0.
 * For the parity tests (a silent gather copy decodes the same tokens) and for serving code
 * sizing its sampled batches; the reference has no counterpart (faster-whisper hides
 * CTranslate2's batching, transcriber.py:53-57).
 */
#define JANUS_ENC_ROWS_OWN      0
#define JANUS_ENC_ROWS_IN_PLACE 1
#define JANUS_ENC_ROWS_GATHERED 2
int janus_whisper_decode_path(janus_whisper* w, int32_t* enc_rows, int32_t* persistent);

/*
 * Where each of the `batch` row slots stands after the last completed decode call (the
 * first position a staggered call may continue it from: tokens and KV rows below it are
 * written). Fails when the last call had another batch size or failed. The continuous-
 * batching plan of the serving step (janus_amd/pipeline.py stagger_plan) continues from
 * here; the reference has no counterpart (its decode is one faster-whisper call per
 * window, transcriber.py:53-57).
 */
int janus_whisper_decode_stand(janus_whisper* w, int32_t* stand, int batch);
/* The same for decoder state slot `slot` (janus_decode_options.state_slot). */
/*
 * A call with janus_decode_options.check_every = 0 (no early-exit polling) returns as soon
 * as its work is enqueued, without waiting for the stream; the persistent segments' grid
 * barrier timeout (a resident grid that never became co-resident) is then reported here:
 * waits for the last such call of state slot `slot` and returns non-zero (janus_last_error)
 * if it timed out — call it before using that call's outputs. The lane's next decode call
 * checks it too. Returns 0 when nothing is pending.
 */
int janus_whisper_decode_check(janus_whisper* w, int slot);
int janus_whisper_decode_stand_slot(janus_whisper* w, int slot, int32_t* stand, int batch);

/*
 * Word-level timestamps: the alignment pass behind faster-whisper's
 * transcribe(word_timestamps=True) (WhisperModel.find_alignment -> CTranslate2
 * Whisper.align; transcriber.py:53-57 with that option). CTranslate2's align cannot be pinned
 * offline; the rule built here, per window, from the window's encoder output enc [1500][d],
 * its content size `size` in mel frames and its text tokens `text` (ids < eot, all the
 * window's segments concatenated, len(text) >= 1):
 *  1. seq = sot_sequence + [<|notimestamps|>] + text + [eot], n tokens. The decoder runs over
 *     seq teacher-forced (causal self-attention, cross-attention over all 1500 frames), fp16
 *     weights, fp32 accumulation.
 *  2. Alignment heads: every head of the last half of the decoder layers (l >= dec_layers / 2;
 *     CTranslate2's default for a checkpoint that names none) unless
 *     janus_whisper_set_alignment_heads named others.
 *  3. Per alignment head, P[h][i][t] = softmax over all 1500 frames of row i's scaled
 *     cross-attention scores. Frames t < F = size / 2 are kept; per head and frame the n rows
 *     are normalised, (P - mean) / std with the population standard deviation; a median
 *     filter of width 7 runs along the frames with reflect padding by 3 (F <= 3: no filter);
 *     the heads are averaged; rows len(sot_sequence) .. n - 2 are kept: A [N][F],
 *     N = len(text) + 1, row r being the step that predicts (text + [eot])[r].
 *  4. DTW on x = -A, fp32, OpenAI's formulation: cost[0][0] = 0, the rest of the border +inf;
 *     cost[i][j] = x[i-1][j-1] + min(c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]);
 *     trace = 0 if c0 < c1 and c0 < c2, else 1 if c1 < c0 and c1 < c2, else 2. Backtrace from
 *     (N, F) with trace[0][*] = 2 and trace[*][0] = 1: 0 moves to (i-1, j-1), 1 to (i-1, j),
 *     2 to (i, j-1); (i-1, j-1) is emitted before each move and the list reversed:
 *     text_indices / time_indices of length L <= N + F. The additions and comparisons run in
 *     exactly this order, so the path of a given matrix is exact, ties included.
 *  5. token_probs[r] = softmax over ids [0, eot) of the logits of row len(sot_sequence) + r,
 *     taken at text[r], r < len(text).
 * Words, their times (time_indices * 0.02 s at the jumps of text_indices) and faster-whisper's
 * add_word_timestamps / seek rules are host code: janus_amd/services/transcriber.py,
 * DESIGN.md §5l.
 *
 * janus_whisper_align, several windows of different lengths in one call:
 *   enc            [device] fp16 [n_enc][1500][d]
 *   tokens         [host] int32 [n_windows][stride]: window w's seq in its first token_lens[w]
 *                  entries; token_lens [host] int32 [n_windows], sot_len + 3 <= n <= n_text_ctx
 *   sizes          [host] int32 [n_windows], each in [2, 3000]
 *   enc_index      [host] int32 [n_windows] (nullable: window w attends to enc row w), as
 *                  janus_decode_rows.enc_index
 *   sot_len, eot   len(sot_sequence) and the <|endoftext|> id
 *   text_indices, time_indices [device] int32 [n_windows][path_stride] (-1 past a window's
 *                  path; path_stride >= every window's N + F), path_lens [device] int32
 *                  [n_windows]
 *   token_probs    [device] f32 [n_windows][stride]: rule 5 in the first len(text) entries of
 *                  each row, 0 after
 *   attn_out       [device] f32, nullable: every window's A [N][F], the windows back to back
 *   phases         0 = the whole call; a mask of 1 (decoder forward and token_probs), 2 (A
 *                  from the kept probabilities) and 4 (DTW) runs those parts alone over what
 *                  the previous call of the same shape left in the context's workspace
 *                  (measurement only)
 * The call allocates from the context's workspace, uses no decoder state slot (it may run
 * between two staggered decode calls) and rejects (non-zero status) a sequence longer than
 * n_text_ctx, a window without text, a size outside [2, 3000] or a token id out of range.
 *
 * janus_whisper_set_alignment_heads: pairs [host] int32 [n_pairs][2] = (layer, head),
 * 1 .. 64 distinct pairs in range; pairs NULL with n_pairs 0 restores the default of rule 2.
 */
int janus_whisper_set_alignment_heads(janus_whisper* w, const int32_t* pairs, int n_pairs);
int janus_whisper_align(janus_whisper* w, const uint16_t* enc, int n_enc, int n_windows,
                        const int32_t* tokens, const int32_t* token_lens, int stride,
                        const int32_t* sizes, const int32_t* enc_index, int sot_len, int eot,
                        int32_t* text_indices, int32_t* time_indices, int32_t* path_lens,
                        int path_stride, float* token_probs, float* attn_out, int phases,
                        void* stream);

/*
 * Language identification for the multilingual models (faster-whisper's language=None /
 * WhisperModel.detect_language -> CTranslate2 Whisper.detect_language). CTranslate2's
 * detect_language cannot be pinned offline (parity unpinned, as the beam and alignment rules
 * above); the rule built here, as CTranslate2's is publicly described, per window:
 *  1. One decoder position holding <|startoftranscript|> (sot_token) at position 0 runs over
 *     the window's encoder output enc [1500][d] (self-attention over itself, cross-attention
 *     over all 1500 frames; fp16 weights, fp32 accumulation — the decode call's kernels).
 *  2. The final LayerNorm of its fp32 residual row, in fp32.
 *  3. Logits for the n_lang language tokens only: the row against embedding rows lang_begin ..
 *     lang_begin + n_lang - 1 (fp16 weights, fp32 products and sums).
 *  4. probs = the fp32 softmax over those n_lang logits (no other token takes part).
 *  5. best = the argmax, the lowest index on ties.
 * enc [device] fp16 [batch][1500][d]; probs [device] f32 [batch][n_lang]; best [device] int32
 * [batch] (an index into the language tokens, not a token id). Any batch >= 1: the call runs
 * chunks of 64 windows. It runs through the decode call's plan and kernels on a lane of its
 * own — no decoder state slot (KV cache, tokens, graphs, stand) is disturbed, so it may run
 * between two staggered decode calls — and replaces the vocabulary projection by a head that
 * reads n_lang x d x 2 bytes of the embedding. 1 <= n_lang <= 128, lang_begin + n_lang <=
 * n_vocab, else non-zero status (janus_last_error). The 99-language models pass lang_begin
 * 50259, n_lang 99; the large-v3 family (n_vocab 51866) n_lang 100 — openai/whisper's order
 * with <|yue|> appended at index 99, token 50358. The context does not know its tokenizer:
 * a *.en model answers too, meaninglessly; callers gate on the model (janus_amd.whisper
 * WhisperEngine.detect_language raises there).
 */
int janus_whisper_detect_language(janus_whisper* w, const uint16_t* enc, int batch, int sot_token,
                                  int lang_begin, int n_lang, float* probs, int32_t* best,
                                  void* stream);

/* ------------------------------------------------------------ vocoder --- */
/*
 * Local Firefly-GAN decoder (fish-speech HiFiGANGenerator architecture) replacing the
 * Fish Audio cloud TTS call client.tts.convert(text=prompt, format="wav", ...)
 * (backend/services/synthesizer.py:179-203, :235-255). Conditioning is the same
 * "(emotion) text" prompt the reference sends (synthesizer.py:151-177).
 */
typedef struct {
  int latent_dim;       /* 512 */
  int channels;         /* upsample_initial_channel, 512 */
  int n_ups;            /* 5 */
  int up_rates[8];      /* 8, 8, 2, 2, 2 (kernel 2u, padding u/2) */
  int n_kernels;        /* 3 */
  int rb_kernels[4];    /* 3, 7, 11 */
  int n_dilations;      /* 3 */
  int rb_dilations[4];  /* 1, 3, 5 */
  int pre_kernel;       /* 13 */
  int post_kernel;      /* 13 */
  int n_emotions;       /* rows of frontend.emotion_embed */
} janus_vocoder_config;

typedef struct janus_vocoder janus_vocoder;

int janus_vocoder_create(const janus_vocoder_config* cfg, janus_vocoder** out);
int janus_vocoder_destroy(janus_vocoder* v);
/*
 * fp32 [host] parameters by fish-speech generator name (weight norm folded):
 * conv_pre.{weight,bias}, ups.{i}.{weight,bias} ([Cin][Cout][2u]),
 * resblocks.{i}.blocks.{j}.convs{1,2}.{m}.{weight,bias}, conv_post.{weight,bias},
 * plus the front end: frontend.text_embed [256][latent], frontend.emotion_embed
 * [n_emotions][latent].
 */
int janus_vocoder_set_tensor(janus_vocoder* v, const char* name, const float* host,
                             int64_t numel);
/*
 * Prompt -> latents: latents [device] fp16 [B][frames][latent] with frame f of row b =
 * text_embed[prompt byte floor(f*n_b/frames)] + emotion_embed[emotion_ids[b]].
 * bytes [device] u8 prompts back to back, byte_offsets [device] int64[B+1],
 * emotion_ids [device] int32[B].
 */
int janus_vocoder_frontend(janus_vocoder* v, const uint8_t* bytes, const int64_t* byte_offsets,
                           const int32_t* emotion_ids, int batch, int frames, uint16_t* latents,
                           void* stream);
/*
 * Same, plus a per-row voice term: latent += speaker[b] ([device] f32 [B][latent], or NULL
 * for none). The voice stands in for the reference's voice cloning, which sends the
 * hot-reloaded recording as references=[ReferenceAudio(audio, text="")] or, without one,
 * reference_id="5196af35..." (synthesizer.py:179-200, :243-249).
 */
int janus_vocoder_frontend_ex(janus_vocoder* v, const uint8_t* bytes, const int64_t* byte_offsets,
                              const int32_t* emotion_ids, const float* speaker, int batch,
                              int frames, uint16_t* latents, void* stream);
/*
 * Voice embedding of reference recordings (the ReferenceAudio bytes of
 * synthesizer.py:183-187, decoded to 16 kHz f32 by the caller): pcm16k [device] f32
 * clips back to back, offsets [device] int64[B+1] (<= 30 s used per clip) ->
 * speaker_out [device] f32 [B][latent] = speaker_bias + speaker_proj . mean over the
 * clip's frames of its normalised Whisper log-mel. Needs the parameters
 * "frontend.speaker_proj" [latent][80], "frontend.speaker_bias" [latent], "mel.basis"
 * and "mel.filters" (as for janus_whisper_set_tensor).
 */
int janus_vocoder_speaker(janus_vocoder* v, const float* pcm16k, const int64_t* offsets, int batch,
                          float* speaker_out, void* stream);
/*
 * Generator forward: latents [device] fp16 [B][frames][latent] -> wav [device] f32
 * [B][frames*prod(up_rates)] in [-1, 1] and, if pcm != NULL, int16 [B][...]
 * (clip(round(32767*y))).
 */
int janus_vocoder_forward(janus_vocoder* v, const uint16_t* latents, int batch, int frames,
                          float* wav, int16_t* pcm, void* stream);
/* Same, plus pre_tanh [device] f32 [B][samples] (conv_post output before tanh; may be NULL). */
int janus_vocoder_forward_ex(janus_vocoder* v, const uint16_t* latents, int batch, int frames,
                             float* wav, int16_t* pcm, float* pre_tanh, void* stream);
/* HIP-event timing of every conv launch (for roofline accounting). */
int janus_vocoder_set_timing(janus_vocoder* v, int on);
/* Accumulated conv FLOPs (2*Cin*Cout*taps*rows), kernel milliseconds and launches. */
int janus_vocoder_conv_stats(janus_vocoder* v, double* flops, double* ms, int64_t* launches,
                             int reset);
/*
 * The same per family: fam[i] = channel width C of the fused ResBlock1 units (4*C*C*k
 * FLOP and 2-3 x C x 2 B of activations per row), or 0 for the conv kernel (conv_pre and
 * the upsamplers). Up to cap families; *n = how many were written. Algorithmic bytes:
 * fp16 activations read once and written once (+ the accumulator / residual reads).
 */
int janus_vocoder_family_stats(janus_vocoder* v, int cap, int* fam, double* flops, double* bytes,
                               double* ms, int64_t* launches, int* n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* JANUS_H_ */

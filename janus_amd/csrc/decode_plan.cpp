// plan_decode: the checks and decisions of one decode call (decode_plan.h). Host only.
#include <algorithm>
#include <sstream>
#include "decode_plan.h"
#include "errors.h"

namespace janus {

// Rows sharing an encoder row (janus_decode_rows::enc_index): how they reach it
// (P.enc_rows) and, read in place, the PAIR / GROUP / ROWS blocks of the absorbed
// cross-attention (P.pairs / P.groups).
static void plan_shared_rows(DecodePlan& P, const janus_whisper_config& c, uint32_t pf,
                             const janus_decode_rows* rows) {
  const int d = c.d_model, H = c.n_heads, B = P.B;
  auto path = [pf](uint32_t f) { return (pf & f) != 0; };
  // shared encoder rows (janus_decode_rows::enc_index): row b attends to enc_in row
  // enc_index[b] of n_enc; the absorbed cross-attention then reads each shared row once per
  // pair of decoder rows (xattn PAIR blocks), other paths get a per-row gathered copy
  const bool shared = rows && rows->enc_index;
  const int n_enc = shared ? rows->n_enc : B;
  if (shared) {
    JANUS_CHECK(n_enc >= 1, "decode: enc_index needs n_enc >= 1");
    for (int b = 0; b < B; ++b)
      JANUS_CHECK(rows->enc_index[b] >= 0 && rows->enc_index[b] < n_enc, "decode: enc_index out of range");
  }
  // (H <= 8, d <= 512: PAIR blocks, the default there. The 12-head family at d = 768 —
  // `wide` — has blocks of up to two or four rows, xattn_rows_kernel, behind
  // JANUS_DEC_PATH_XROWS(n): measured SLOWER than the gathered copies at 320 rows, DESIGN.md
  // §5i, so without the flag its shared rows are gathered)
  const bool wide = P.wide = !(H <= 8 && d <= 512);
  const int xrows = 2 * (int)((pf >> 18) & 3u);   // JANUS_DEC_PATH_XROWS(n): n = 2 or 4, 0 = off
  JANUS_CHECK(xrows == 0 || (xattn_rows_supported(d, H) && xrows <= xattn_rows_max(d, H)),
              "decode: JANUS_DEC_PATH_XROWS(n) is n = 2 or 4 rows per block at 12 heads, d_model 768");
  const bool pair_ok = shared && xattn_supported(d, H) && (!wide || xrows > 0) &&
                       B <= kSkinnyMaxRows && !path(JANUS_DEC_PATH_NO_XABSORB) && !path(JANUS_DEC_PATH_NO_XPAIR);
  JANUS_CHECK(!(wide && path(JANUS_DEC_PATH_XGROUP)),
              "decode: JANUS_DEC_PATH_XGROUP (GROUP blocks of 8-head rows) needs H <= 8, d <= 512");
  P.enc_rows = !shared ? JANUS_ENC_ROWS_OWN : pair_ok ? JANUS_ENC_ROWS_IN_PLACE : JANUS_ENC_ROWS_GATHERED;
  P.n_enc = pair_ok ? n_enc : B;
  // rows sharing an encoder row (best_of = 5 hypotheses of a window): PAIR blocks
  // (xattn_kernel<PAIR>, two blocks per CU, the window's output read once per two rows).
  // GROUP blocks of up to 6 rows (xattn_group_kernel: one read for all hypotheses) are
  // opt-in, JANUS_XGROUP=1: measured slower in the fallback step (4 810 vs 4 380 ms per
  // step, two same-box pairs, profiles/r04_lanes_sweep_fallback_ab.json) — one block per
  // CU with three m-tiles of queries staged through LDS loses more than the reads it saves
  std::vector<int>& h_groups = P.groups;
  int& grp_rows = P.grp_rows;
  int& rem_rows = P.rem_rows;
  if (!pair_ok) return;
  std::vector<std::vector<int>> grp(n_enc);
  for (int b = 0; b < B; ++b) grp[rows->enc_index[b]].push_back(b);
  size_t maxg = 0;
  for (auto& g : grp) maxg = std::max(maxg, g.size());
  if (wide) {
    // blocks of up to xrows rows of one encoder row, in row order (4: best_of = 5 is 4 + 1)
    grp_rows = (int)std::min<size_t>((size_t)xrows, maxg);
    // each encoder row's remainder rows (fewer than a full block) go out as blocks of a
    // second launch with their own, smaller m-tile count (a lone row: one m-tile, two blocks
    // per CU): 5 493 -> 4 496 us per position at 320 rows on small.en against keeping them
    // in the full blocks' launch, DESIGN.md §5i
    std::vector<int> rem;
    for (int e = 0; e < n_enc; ++e)
      for (size_t i = 0; i < grp[e].size(); i += grp_rows) {
        const size_t n = std::min<size_t>(grp_rows, grp[e].size() - i);
        std::vector<int>& dst = (int)n < grp_rows ? rem : h_groups;
        if (&dst == &rem) rem_rows = std::max(rem_rows, (int)n);
        dst.push_back(e);
        for (int j = 0; j < 7; ++j) dst.push_back(j < (int)n ? grp[e][i + j] : -1);
      }
    P.n_main = (int)h_groups.size() / 8;
    h_groups.insert(h_groups.end(), rem.begin(), rem.end());
  } else if (maxg > 2 && path(JANUS_DEC_PATH_XGROUP)) {
    grp_rows = (int)std::min<size_t>(6, maxg);
    for (int e = 0; e < n_enc; ++e)
      for (size_t i = 0; i < grp[e].size(); i += grp_rows) {
        h_groups.push_back(e);
        for (int j = 0; j < 7; ++j)
          h_groups.push_back(j < grp_rows && i + j < grp[e].size() ? grp[e][i + j] : -1);
      }
  } else {
    // rows grouped by encoder row, paired in row order within a group
    for (int e = 0; e < n_enc; ++e)
      for (size_t i = 0; i < grp[e].size(); i += 2)
        P.pairs.push_back(XPair{grp[e][i], i + 1 < grp[e].size() ? grp[e][i + 1] : -1, e, 0});
  }
}

// The rows' prompts, the staggered rows' offsets and the positions the call runs; the
// beam-search and continuation rejections.
static void plan_rows(DecodePlan& P, const janus_whisper_config& c, const janus_decode_options& opt,
                      const janus_decode_rows* rows, const DecodeSampling* smp, const BeamMode* beam,
                      const LaneStand& stand) {
  const int B = P.B, maxlen = P.maxlen, NC = c.n_text_ctx;
  // per-row prompts (janus_decode_rows): row b samples from position plen[b]; all rows step
  // together from position 0, rows still inside their prompt keep the forced token
  const bool per_row = rows && rows->prompts;
  std::vector<int32_t>& h_plen = P.plen;
  std::vector<int32_t>& h_init = P.init;
  h_plen.assign(B, opt.prompt_len);
  h_init.assign((size_t)B * maxlen, -1);
  if (per_row) {
    JANUS_CHECK(rows->prompt_lens && rows->stride >= 1, "decode: per-row prompts need lengths and a stride");
    for (int b = 0; b < B; ++b) {
      h_plen[b] = rows->prompt_lens[b];
      JANUS_CHECK(h_plen[b] >= 1 && h_plen[b] <= rows->stride && h_plen[b] < maxlen,
                  "decode: per-row prompt length out of range");
      for (int i = 0; i < h_plen[b]; ++i) h_init[(size_t)b * maxlen + i] = rows->prompts[(size_t)b * rows->stride + i];
    }
  } else {
    JANUS_CHECK(opt.prompt && opt.prompt_len >= 1, "decode: missing prompt");
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < opt.prompt_len; ++i) h_init[(size_t)b * maxlen + i] = opt.prompt[i];
  }
  // staggered rows (janus_decode_rows.pos_offset): rows with an offset > 0 continue the
  // previous call's state in the same slots (tokens, KV cache, counters, rule state); rows
  // with 0 start fresh and must be one contiguous range [f0, f1). Every row runs `steps`
  // positions from its own offset.
  const bool stagger = rows && rows->pos_offset;
  int &f0 = P.f0, &f1 = P.f1, &max_roff = P.max_roff;
  f0 = 0; f1 = B; max_roff = 0;
  std::vector<int32_t>& h_roff = P.roff;
  if (stagger) {
    JANUS_CHECK(!P.shared() && !(smp && smp->temperature > 0.f), "decode: staggered rows are greedy, unshared");
    h_roff.assign(rows->pos_offset, rows->pos_offset + B);
    f0 = B; f1 = 0;
    for (int b = 0; b < B; ++b) {
      JANUS_CHECK(h_roff[b] >= 0 && h_roff[b] < maxlen, "decode: pos_offset out of range");
      max_roff = std::max(max_roff, h_roff[b]);
      if (h_roff[b] == 0) { f0 = std::min(f0, b); f1 = std::max(f1, b + 1); }
    }
    if (f1 <= f0) f0 = f1 = 0;
    for (int b = f0; b < f1; ++b) JANUS_CHECK(h_roff[b] == 0, "decode: fresh rows must be contiguous");
  }
  if (beam) {
    JANUS_CHECK(c.d_model <= 768, "decode: beam search needs d_model <= 768 (the vocabulary projection has no "
                                  "beam partials at 1280)");
    JANUS_CHECK(beam->k >= 1 && beam->k <= kBeamMax && B % beam->k == 0, "decode: beam_size must be 1 .. 8");
    JANUS_CHECK(!stagger, "decode: beam search does not take staggered rows (pos_offset)");
    JANUS_CHECK(!(smp && smp->temperature > 0.f), "decode: beam search runs at temperature 0");
    JANUS_CHECK(B <= kSkinnyMaxRows, "decode: windows x beam_size must be <= 512 rows");
    JANUS_CHECK(per_row && maxlen <= 448, "decode: beam search needs per-row prompts, max_length <= 448");
    P.beam_k = beam->k;
    P.nwin = B / beam->k;
  }
  // history rules (janus_decode_options, rule at include/janus.h): a penalty of 0 or 1 and n = 0 are off
  {
    const float p = opt.repetition_penalty;
    const int n = opt.no_repeat_ngram_size;
    JANUS_CHECK(p >= 0.f, "decode: repetition_penalty must be > 0 (0 or 1: off)");   // (NaN fails too)
    JANUS_CHECK(n >= 0, "decode: no_repeat_ngram_size must be >= 0");
    P.rep_pen = p == 0.f ? 1.f : p;
    P.ngram = n;
    if (P.hist()) {
      JANUS_CHECK(!beam, "decode: beam search takes no repetition_penalty / no_repeat_ngram_size");
      JANUS_CHECK(!stagger, "decode: staggered rows (pos_offset) take no repetition_penalty / no_repeat_ngram_size");
    }
  }
  JANUS_CHECK(!stagger || rows->steps >= 0, "decode: steps must be >= 0");
  P.steps = (stagger && rows->steps > 0) ? rows->steps : maxlen - 1;
  JANUS_CHECK(!stagger || max_roff + P.steps <= maxlen, "decode: pos_offset + steps > max_length");
  // a continuing row reads the tokens and KV rows its slot holds: only up to where the
  // previous calls left it (a larger offset would read unwritten tokens / KV rows)
  if (stagger) {
    for (int b = 0; b < B; ++b) {
      if (h_roff[b] == 0) continue;
      JANUS_CHECK((int)stand.stand->size() == B && stand.maxlen == maxlen,
                  "decode: continuing rows need the previous call's batch size and max_length");
      JANUS_CHECK(h_roff[b] <= (*stand.stand)[b],
                  "decode: row " + std::to_string(b) + " continues at pos_offset " + std::to_string(h_roff[b]) +
                      " but its slot stands at " + std::to_string((*stand.stand)[b]));
    }
  }
  const int min_plen = f1 > f0 ? *std::min_element(h_plen.begin() + f0, h_plen.begin() + f1) : 1;
  const int max_plen = f1 > f0 ? *std::max_element(h_plen.begin() + f0, h_plen.begin() + f1) : 1;
  JANUS_CHECK(min_plen >= 1 && max_plen < maxlen && maxlen <= NC,
              "decode: need 1 <= prompt_len < max_length <= n_text_ctx");
  // no_speech_prob read no_speech_back positions before each row's last prompt position (the
  // <|startoftranscript|> position of a [sot, language, task] prompt): inside every prompt
  const int back = P.nsp_back = rows ? rows->no_speech_back : 0;
  for (int b = 0; b < B; ++b)
    JANUS_CHECK(back >= 0 && back < h_plen[b], "decode: need 0 <= no_speech_back < prompt_len in every row");
  // index of the first position whose logits are read — the first sampled token, or the
  // earliest no-speech position before it (earliest row): the vocabulary projection runs from
  // there on; staggered continuing rows sample from the first step on
  P.sample_begin = (stagger && f1 - f0 < B) ? 0 : min_plen - (f1 > f0 ? back : 0);
}

// Sampling: the rules' temperature and the per-row 1 / T.
static void plan_sampling(DecodePlan& P, const janus_decode_options& opt, const janus_decode_rows* rows,
                          const DecodeSampling* smp) {
  const bool sampling = P.sampling = smp && smp->temperature > 0.f;
  if (sampling) JANUS_CHECK(smp->seeds, "decode: sampling needs per-row seeds");
  P.row_temps = sampling && smp->temps;
  if (P.row_temps) {
    P.itemp.resize(P.B);
    for (int b = 0; b < P.B; ++b) {
      JANUS_CHECK(smp->temps[b] >= 0.f, "decode: per-row temperatures must be >= 0");
      P.itemp[b] = smp->temps[b] > 0.f ? 1.0f / smp->temps[b] : 0.f;   // 0: a greedy row
    }
  }
  DecodeRules& R = P.R;
  R.eot = opt.eot;
  R.suppress_blank = opt.suppress_blank;
  R.blank = opt.blank_token;
  R.ts_begin = opt.timestamp_begin;
  R.no_timestamps = opt.no_timestamps;
  R.max_initial_ts = opt.max_initial_timestamp_index;
  R.target = rows ? rows->no_speech_token : -1;
  R.target_back = P.nsp_back;
  // per-row temperatures: R.inv_temp only selects the sampling kernel (rows read their own)
  R.inv_temp = !sampling ? 0.f : smp->temps ? 1.0f : 1.0f / smp->temperature;
}

// Which kernels a position launches: the cross-attention form, the LayerNorm placements,
// the fused merge / select, the persistent level.
static void plan_paths(DecodePlan& P, const janus_whisper_config& c, const janus_decode_options& opt,
                       bool multi_lane, const SegDevice& seg) {
  const int d = c.d_model, H = c.n_heads, Te = c.n_audio_ctx, V = c.n_vocab, B = P.B;
  const uint32_t pf = opt.path_flags;
  auto path = [pf](uint32_t f) { return (pf & f) != 0; };
  const int cus = P.cus;
  // launch geometry from the options (janus_decode_options.logits_blocks / msplit_rows_n;
  // measured defaults: DESIGN.md §5b / §5d)
  P.lg_cap = opt.logits_blocks > 0 ? opt.logits_blocks : cus;
  P.msplit_n = opt.msplit_rows_n > 0 ? opt.msplit_rows_n
               : opt.msplit_rows_n < 0 ? 0 : (cus <= 128 ? 1024 : 0);
  P.nblk = logits_partial_blocks(V, d, P.lg_cap);
  // cross-attention: absorbed (stream enc itself, JANUS_DEC_PATH_NO_XABSORB restores per-layer K/V)
  const bool xabs = P.xabs = xattn_supported(d, H) && B <= kSkinnyMaxRows && !path(JANUS_DEC_PATH_NO_XABSORB);
  const int xsplit = P.xsplit = xattn_split_count(Te, opt.xattn_splits);
  // JANUS_DEC_PATH_FUSED_LN (B <= 64): LayerNorm rides on the projections (row-statistic pieces
  // written by the producer of each residual row, normalised on load by the consumer).
  // Opt-in: with the 16-wave skinny GEMM the separate LayerNorm launch measured faster
  // (637.7 vs 660.8 ms per bench step) — the consumer ingests A as fp32.
  // (the int8 decoder weights, i8 below, have no LayerNorm-on-load, resid_ln or merge + value
  // projection form: every layer runs unfused, as the models above d_model 512 run it)
  const bool i8 = P.dec_i8;
  const bool fused_ln = P.fused_ln = B <= 64 && !i8 && path(JANUS_DEC_PATH_FUSED_LN);
  // JANUS_DEC_PATH_LN_FUSE (opt-in, B <= 64): LayerNorm handed off inside the producing kernel —
  // the residual GEMM's last block normalises the new rows (GemmArgs::ln_out, sc1 stores
  // + arrival counter), the embedding kernel normalises its row; no LayerNorm launches.
  // Measured slower than the separate launches (616.8 vs 536.5 ms per bench step): the
  // write-through stores and the serial tail cost more than the launch they save.
  const bool ln_fuse = P.ln_fuse = B <= 64 && !i8 && !fused_ln && d <= 512 && path(JANUS_DEC_PATH_LN_FUSE);
  // LayerNorm in the consuming projection's prologue (GemmArgs::lnin_x: each block
  // normalises its rows of x into an fp16 LDS tile; the vocabulary projection the final
  // LayerNorm) instead of a LayerNorm launch.
  // Per LayerNorm (bit mask, JANUS_DEC_PATH_LN_MASK(m) overrides): 1 = LN1 into the QKV
  // projection, 2 = LN2 into the absorbed query projection, 4 = LN3 into fc1, 8 = the final
  // LayerNorm into the vocabulary projection. Measured per kernel, decoder alone on 16 CUs
  // per XCD: QKV 9.2 us vs 5.6 + 5.1 (LayerNorm launch), fc1 8.6 vs 5.2 + 5.1, logits 49.4
  // vs 47.3 + 5.1 — but the absorbed query projection 16.1 vs 9.2 + 5.1 us: its 256
  // 64-row blocks would each normalise all 64 rows. Beside the vocoder (overlapped
  // step, decoder side): mask 0 303.5-308.7, 13 305.1-306.8, 9 304.0-304.2, 5 306.6-306.9
  // ms — within the box's noise; 9 (LN1 + final) is the default up to 64 rows. Above (the
  // staggered 2 x 64 rows) every LayerNorm is its own launch: decoder side 230-234 ms with
  // mask 0 against 235-241 (9), 245-249 (13), 265-269 (15) on one box
  // (profiles/r04_decoder_knobs.json): each prologue normalises its block's rows again.
  P.ln_pro_mask = (B <= kSkinnyMaxRows && d <= 512 && !i8 && !fused_ln && !ln_fuse)
                      ? (path(JANUS_DEC_PATH_LN_PROLOGUE) ? (int)((pf >> 12) & 15u)
                                                          : (B <= 64 ? 9 : 0))
                      : 0;
  // the embedding kernel owns whole rows (one block per utterance): it also writes the
  // first layer's LayerNorm of its row, one launch fewer per position
  // (JANUS_NO_EMBED_LN restores the separate launch)
  P.embed_ln = !i8 && !fused_ln && !ln_fuse && d <= 512 && !path(JANUS_DEC_PATH_NO_EMBED_LN);
  // Opt-in (JANUS_DEC_PATH_RESID_LN): the attention output projections and the LayerNorm after
  // them (LN2 / LN3) in one launch (resid_ln_kernel: 16 rows per block over all d columns,
  // bit-identical to the residual GEMM + LayerNorm pair). Measured 72 ms per step SLOWER
  // on the decoder side (361 vs 289 ms): at B = 64 only 4 blocks stream the 0.5 MB weight
  // each, at ~25 GB/s per CU (≈ 24 µs per launch against 5.6 + 5.0 µs for the pair).
  const bool rln = P.rln = B <= 64 && !i8 && !fused_ln && !ln_fuse && resid_ln_supported(d, d) &&
                           path(JANUS_DEC_PATH_RESID_LN);
  // the split merge fused into the per-head value projection (one launch) up to 64 rows;
  // above (the staggered 2 x 64 rows) the merge in the cross-attention's last split block
  // and a block-diagonal skinny projection measured faster (decoder side -1.5 / -2.9 ms
  // per step on two boxes, profiles/r04_decoder_knobs.json); bit-identical either way
  // (xattn_combine_vproj_kernel; JANUS_DEC_PATH_NO_CVP / _CVP force either form)
  P.cvp = !i8 && xattn_cvp_supported(d, H) && xsplit <= 16 && !path(JANUS_DEC_PATH_NO_CVP) &&
          (B <= 64 || P.ngroups() > 0 || path(JANUS_DEC_PATH_CVP));
  // the selection at pos and the embedding at pos + 1 in one launch (select_embed_kernel,
  // bit-identical; JANUS_DEC_PATH_NO_SEL_EMBED restores the two launches): a step from the first
  // sampled position on finds its row already embedded by the previous step's selection
  // (beam search: the beam step picks the tokens, the next position embeds them itself)
  P.fuse_se = !path(JANUS_DEC_PATH_NO_SEL_EMBED) && !P.beam_k;
  JANUS_CHECK(!P.stagger() || (!fused_ln && !ln_fuse && !rln && xabs),
              "decode: staggered rows run the default decoder kernels only");
  JANUS_CHECK(!P.stagger() || B <= kSkinnyMaxRows, "decode: staggered rows need B <= kSkinnyMaxRows");
  JANUS_CHECK(!(xabs && P.ngroups() > 0) || P.cvp || P.wide,
              "decode: shared-encoder groups need the fused merge (no JANUS_DEC_PATH_NO_CVP)");
  // persistent segments (dec_persist.hip, janus_decode_options.persistent): per layer the
  // launches between the self-attention and the cross-attention (O + residual, LN2, the
  // absorbed query projection) and between the cross-attention and the next layer's
  // self-attention (value projection, cross O + residual, LN3, fc1, fc2 + residual, LN1,
  // QKV) as two resident grids; the cross-attention then runs at one key split (its
  // output written directly). Shapes it does not cover keep the launch path.
  // (resident grids need every block co-resident: the kernels' occupancy must admit one
  // block per CU of the partition, and a multi-lane call, whose lanes run concurrently on
  // the same CUs, keeps the launch path)
  // (beam search runs the launch path: a persistent request falls back, as at d_model 768;
  // so does a call with history rules)
  // (the int8 cross-attention likewise: the persistent levels' one-split forms are not built for it;
  // and the int8 decoder weights: the segments multiply the fp16 weights)
  const int seg_grid = P.seg_grid =
      opt.persistent && !multi_lane && !P.beam_k && !P.hist() && !P.cross_i8 && !i8
          ? seg.grid(B, cus, path(JANUS_DEC_PATH_SEG_2CU)) : 0;
  const bool persist = seg_grid > 0 && dec_seg_supported(d, H, B, cus) && seg.resident(seg_grid, cus) &&
                       xabs && !P.shared() && !fused_ln && !ln_fuse && !rln && P.ngroups() == 0 && P.npairs() == 0;
  // persistent = 2: segment B of layer l, the self-attention of l + 1 and its segment A as
  // ONE launch per layer step (dec_layer_kernel): 29 -> 19 launches per position; layer
  // 0's QKV, self-attention and segment A as one head kernel and the final LayerNorm as the
  // last segment B's phase: 16
  const bool layerk = persist && opt.persistent >= 2 && 2 * ((B + 1) / 2) <= 2 * seg_grid;
  // persistent = 3: the cross-attention as the head / layer kernel's last phase (10 launches
  // per position); the decoder side measured level with 16 (369.1-369.3 vs 368.4-369.4 ms
  // over 447 positions, profiles/r05_xattn_phase_ab.txt): a grid barrier costs what the
  // launch boundary it replaces did
  const bool xfuse = layerk && opt.persistent >= 3 && B <= 2 * seg_grid;
  P.persist = (int)persist + (int)layerk + (int)xfuse;
  // odd layers' cross-attention sweeps the encoder output's key chunks last to first, so it
  // starts on what the layer before it read last, still in the Infinity Cache (at 256 rows a
  // layer reads 393 MB, past its 256 MB): decoder 1472 -> 1394 us per position in the
  // staggered step (profiles/r06_xattn_ab.txt); JANUS_DEC_PATH_XFWD keeps every sweep forwards
  // (only the persistent levels' one-split cross-attention sweeps either way)
  P.xrev = persist && !path(JANUS_DEC_PATH_XFWD);
  P.use_graph = !path(JANUS_DEC_PATH_NO_GRAPH);
}

DecodePlan plan_decode(const janus_whisper_config& cfg, const janus_decode_options& opt,
                       const janus_decode_rows* rows, const DecodeSampling* smp, const BeamMode* beam,
                       int B, int cus, bool multi_lane, const LaneStand& stand, const SegDevice& seg,
                       int cross_compute, int dec_compute) {
  DecodePlan P;
  P.B = B;
  // int8 decoder weights (janus_whisper_set_decoder_compute): greedy and sampled calls on the
  // absorbed launch path
  JANUS_CHECK(dec_compute == JANUS_DEC_COMPUTE_F16 || dec_compute == JANUS_DEC_COMPUTE_INT8,
              "decode: decoder_compute must be 0 (float16) or 1 (int8)");
  if ((P.dec_i8 = dec_compute == JANUS_DEC_COMPUTE_INT8)) {
    const uint32_t pf = opt.path_flags;
    JANUS_CHECK(!beam, "decode: beam search with decoder_compute int8: the beam partials of the vocabulary "
                       "projection read the fp16 table only");
    JANUS_CHECK(!(pf & JANUS_DEC_PATH_NO_XABSORB),
                "decode: JANUS_DEC_PATH_NO_XABSORB with decoder_compute int8: the per-layer cross K / V and "
                "query projections have no int8 weights");
    JANUS_CHECK(!(pf & JANUS_DEC_PATH_XGROUP),
                "decode: JANUS_DEC_PATH_XGROUP with decoder_compute int8: GROUP blocks need the fused merge + "
                "value projection, which reads the fp16 weights only");
    JANUS_CHECK(xattn_supported(cfg.d_model, cfg.n_heads) && B <= kSkinnyMaxRows,
                "decode: decoder_compute int8 needs the absorbed cross-attention (d_model 384 .. 1280, <= 512 rows)");
  }
  // int8 cross-attention (janus_whisper_set_cross_compute): the absorbed launch path's one-row,
  // PAIR and one-split forms only
  JANUS_CHECK(cross_compute == JANUS_CROSS_COMPUTE_F16 || cross_compute == JANUS_CROSS_COMPUTE_INT8,
              "decode: cross_compute must be 0 (float16) or 1 (int8)");
  if ((P.cross_i8 = cross_compute == JANUS_CROSS_COMPUTE_INT8)) {
    const uint32_t pf = opt.path_flags;
    JANUS_CHECK(!(pf & JANUS_DEC_PATH_NO_XABSORB),
                "decode: JANUS_DEC_PATH_NO_XABSORB with cross_compute int8: the int8 encoder output is read by "
                "the absorbed cross-attention only");
    JANUS_CHECK(!(pf & JANUS_DEC_PATH_XGROUP),
                "decode: JANUS_DEC_PATH_XGROUP with cross_compute int8: GROUP blocks read the fp16 encoder output only");
    JANUS_CHECK(!((pf >> 18) & 3u),
                "decode: JANUS_DEC_PATH_XROWS with cross_compute int8: ROWS blocks read the fp16 encoder output only");
    JANUS_CHECK(xattn_supported(cfg.d_model, cfg.n_heads) && B <= kSkinnyMaxRows,
                "decode: cross_compute int8 needs the absorbed cross-attention (d_model 384 .. 1280, <= 512 rows)");
  }
  P.maxlen = opt.max_length;
  P.check_every = opt.check_every;
  P.chunk = opt.check_every > 0 ? opt.check_every : 16;
  // cu_count: the CUs the caller's stream may use (a CU-masked partition); 0 = read it
  // from the stream's CU mask
  // (a caller's cu_count larger than its stream's CU mask is clamped to the mask)
  P.cus = opt.cu_count > 0 ? std::min(opt.cu_count, cus) : cus;
  plan_shared_rows(P, cfg, opt.path_flags, rows);
  plan_rows(P, cfg, opt, rows, smp, beam, stand);
  plan_sampling(P, opt, rows, smp);
  plan_paths(P, cfg, opt, multi_lane, seg);
  return P;
}

std::string DecodePlan::describe() const {
  std::ostringstream o;
  each_scalar([&](const char* n, auto v) { o << n << '=' << +v << '\n'; },
              [&](const char* n, auto v) { o << "call." << n << '=' << +v << '\n'; });
  if (hist()) o << "repetition_penalty=" << rep_pen << "\nno_repeat_ngram_size=" << ngram << '\n';
  if (cross_i8) o << "cross_int8=1\n";
  if (dec_i8) o << "dec_int8=1\n";
  o << "pairs=";
  for (size_t i = 0; i < pairs.size(); ++i)
    o << (i ? "," : "") << pairs[i].b0 << ',' << pairs[i].b1 << ',' << pairs[i].e;
  o << "\ngroups=";
  for (size_t i = 0; i < groups.size(); ++i) o << (i ? "," : "") << groups[i];
  o << '\n';
  return o.str();
}

}  // namespace janus

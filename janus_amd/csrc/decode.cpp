// The Whisper decode call: greedy decoding, temperature sampling and beam search on one or
// several decoder lanes. A call on a lane (decode_lane) is planned first (plan_decode,
// decode_plan.h: every check and every path decision, no device work), then run: the lane's
// buffers (ensure_buffers), the uploads (upload_inputs), the per-layer cross K/V projections
// where the cross-attention is not absorbed, the positions (run_positions: DecodeStep per
// position, captured into graphs keyed by the plan and the buffers) and the outputs (finish).
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <thread>
#include <type_traits>
#include "decoder.h"
#include "dec_persist.h"
#include "decode_plan.h"
#include "whisper_internal.h"

namespace janus {

// Lanes allocate their workspaces (hipMalloc / hipFree) before any of them starts a graph
// capture: every lane arrives here after its allocations, and captures once all have.
struct LaneLatch {
  std::mutex m;
  std::condition_variable cv;
  int left = 0;
  void arrive(bool wait) {
    std::unique_lock<std::mutex> lk(m);
    if (--left == 0) cv.notify_all();
    if (wait) cv.wait(lk, [&] { return left <= 0; });
  }
};
struct LaneArrival {
  LaneLatch* l;
  bool done = false;
  explicit LaneArrival(LaneLatch* latch) : l(latch) {}
  void now() {
    if (l && !done) l->arrive(true);
    done = true;
  }
  ~LaneArrival() {
    if (l && !done) l->arrive(false);  // a lane that failed early must not stall the others
  }
};

// The deferred barrier-timeout check of the lane's last non-polling call (check_every 0):
// waits for that call's flag copy and throws if a persistent segment gave up at a barrier.
static void lane_check(DecLane& Z) {
  if (!Z.segerr_pending) return;
  Z.segerr_pending = false;
  JANUS_HIP(hipEventSynchronize(Z.ev_segerr));
  if (*Z.h_segerr) {
    *Z.h_segerr = 0;
    JANUS_HIP(hipMemset(Z.d_segbar.p, 0, sizeof(unsigned) * 256));
    JANUS_HIP(hipMemset(Z.d_segerr.p, 0, 256));
    throw Error("decode: a persistent decoder segment timed out at a grid barrier (grid not co-resident)");
  }
}

// What the caller handed one lane: its slice of the inputs and where its outputs go.
struct DecodeCall {
  const _Float16* enc_in;
  const janus_decode_options* opt;
  const janus_decode_rows* rows;
  const DecodeSampling* smp;
  const BeamMode* beam;
  int32_t* tokens_out;
  int32_t* n_tokens_out;
  float* sum_lp_out;
  float* nsp_out;
};

// Every device pointer a captured kernel reads, typed. Pointers only: the graph cache key
// takes the struct word for word (append_key), so a buffer added here is in the key.
struct LaneBuffers {
  float* x;
  _Float16 *a, *qkv, *o, *q2, *f;
  _Float16 *kcache, *vcache;     // [layers][B][n_text_ctx][d] self-attention K / V
  _Float16 *ckeys, *cvals;       // [layers][B * Te][d] projected cross K / V (not absorbed)
  float *part_o, *part_ml;
  LogitPart* parts;
  RowRules* rules;
  float2* lnp;
  int* lncnt;
  _Float16 *xqk, *xc;
  float *xpc, *xpml;
  const _Float16* enc;
  int32_t *tokens, *done, *n_tokens, *prompt;
  float *sum_lp, *nsp;
  uint8_t* smask;
  uint32_t* seed;
  float* itemp;
  const int4* xpairs;            // null: no PAIR blocks
  const int* xgroups;            // null: no GROUP / ROWS blocks
  const int32_t* roff;           // null: not staggered
  _Float16* omid;
  unsigned *segbar, *segerr;
  BeamTop* btop;
  int32_t *bint, *bfin;
  float* bfs;
  uint32_t* hist;                // null: no history rules
  const int8_t* encq;            // null: the fp16 encoder output (int8 cross-attention: its rows
  const float* encs;             // quantised, and their per-key scales)

  void append_key(std::vector<int64_t>& key) const {
    static_assert(std::is_trivially_copyable<LaneBuffers>::value && sizeof(LaneBuffers) % sizeof(int64_t) == 0 &&
                      sizeof(void*) == sizeof(int64_t), "LaneBuffers holds pointers only");
    const size_t at = key.size();
    key.resize(at + sizeof(LaneBuffers) / sizeof(int64_t));
    std::memcpy(&key[at], this, sizeof(LaneBuffers));
  }
};

// Sizes the lane's buffers for the plan (grow-only; a reallocation changes the pointer and
// with it the graph key) and returns them typed.
static LaneBuffers ensure_buffers(janus_whisper* w, DecLane& Z, const DecodePlan& P, int n_suppress,
                                  hipStream_t s) {
  const auto& c = w->cfg;
  const int d = c.d_model, H = c.n_heads, Te = c.n_audio_ctx, V = c.n_vocab, NC = c.n_text_ctx;
  const int B = P.B, maxlen = P.maxlen, nl = c.dec_layers;
  const int64_t Me = (int64_t)B * Te;
  // the captured decode graphs bake in every pointer they read: the encoder output goes
  // to a context-owned buffer first (one ~0.1 ms device copy) so the graphs are reused
  // whatever buffer the caller's allocator handed out this time
  if (!P.cross_i8) Z.d_enc.ensure(sizeof(_Float16) * (int64_t)P.n_enc * Te * d);
  if (P.cross_i8) {   // the rows as the cross-attention reads them: int8 and one scale per key
    Z.d_encq.ensure((int64_t)P.n_enc * Te * d);
    Z.d_encs.ensure(sizeof(float) * (int64_t)P.n_enc * Te);
  }
  if (P.npairs() > 0) Z.d_xpairs.ensure(sizeof(int4) * P.npairs());
  if (P.ngroups() > 0) Z.d_xgroups.ensure(sizeof(int) * P.groups.size());
  Z.d_x.ensure(sizeof(float) * B * d);
  Z.d_a.ensure(sizeof(_Float16) * B * d);
  Z.d_qkv.ensure(sizeof(_Float16) * B * 3 * d);
  Z.d_o.ensure(sizeof(_Float16) * B * d);
  Z.d_q2.ensure(sizeof(_Float16) * B * d);
  Z.d_f.ensure(sizeof(_Float16) * B * 4 * d);
  Z.d_kc.ensure(sizeof(_Float16) * (int64_t)nl * B * NC * d);
  Z.d_vc.ensure(sizeof(_Float16) * (int64_t)nl * B * NC * d);

  Z.d_smask.ensure((V + 15) / 16 * 16);  // logits_partial_kernel reads 16 mask bytes per tile
  const int max_split = std::max(decode_split_count(Te), decode_split_count(NC));
  Z.d_part_o.ensure(sizeof(float) * (int64_t)B * max_split * d);
  Z.d_part_ml.ensure(sizeof(float) * (int64_t)B * max_split * H * 2);
  Z.d_parts.ensure(sizeof(LogitPart) * (int64_t)B * P.nblk);
  Z.d_rules.ensure(sizeof(RowRules) * B);
  // beam search: the partials' best entries, the per-window state and the finished list
  if (P.beam_k) {
    Z.d_btop.ensure(sizeof(BeamTop) * (int64_t)B * P.nblk);
    Z.d_bint.ensure(sizeof(int32_t) * (4 * (int64_t)P.nwin + 2 * (int64_t)B));
    Z.d_bfin.ensure(sizeof(int32_t) * (int64_t)B * maxlen);
    Z.d_bfs.ensure(sizeof(float) * B);
  }
  Z.d_done.ensure(sizeof(int32_t) * B);
  Z.d_prompt.ensure(sizeof(int32_t) * B);   // per-row prompt lengths
  Z.d_tok.ensure(sizeof(int32_t) * (int64_t)B * maxlen);
  Z.d_ntok.ensure(sizeof(int32_t) * B);
  Z.d_slp.ensure(sizeof(float) * B);
  Z.d_nsp.ensure(sizeof(float) * B);
  Z.d_supp.ensure(sizeof(int32_t) * (n_suppress > 0 ? n_suppress : 1));
  Z.d_roff.ensure(sizeof(int32_t) * B);
  Z.d_seed.ensure(sizeof(uint32_t) * B);
  if (P.row_temps) Z.d_itemp.ensure(sizeof(float) * B);
  if (P.hist()) Z.d_hist.ensure(sizeof(uint32_t) * history_words(V, d, B));
  if (P.xabs) {
    Z.d_xqk.ensure(sizeof(_Float16) * B * H * d);
    Z.d_xc.ensure(sizeof(_Float16) * B * H * d);
    Z.d_xpc.ensure(sizeof(float) * (int64_t)B * P.xsplit * H * d);
    Z.d_xpml.ensure(sizeof(float) * (int64_t)B * P.xsplit * H * 2);
  }
  // cross-attention keys/values, once per window
  if (!P.xabs) {
    Z.d_ck.ensure(sizeof(_Float16) * (int64_t)nl * Me * d);
    Z.d_cv.ensure(sizeof(_Float16) * (int64_t)nl * Me * d);
  }
  Z.d_lnp.ensure(sizeof(float2) * B * (d / 16));
  Z.d_lncnt.ensure(sizeof(int) * 64);  // one arrival counter per 16-row block (JANUS_DEC_PATH_LN_FUSE)
  if (P.persist) {
    Z.d_omid.ensure(sizeof(_Float16) * B * d);
    if (!Z.d_segbar.p) {  // barrier counters start at zero; the kernels leave them zeroed
      Z.d_segbar.ensure(sizeof(unsigned) * 256);
      JANUS_HIP(hipMemsetAsync(Z.d_segbar.p, 0, sizeof(unsigned) * 256, s));
    }
    if (!Z.d_segerr.p) {
      Z.d_segerr.ensure(256);
      JANUS_HIP(hipMemsetAsync(Z.d_segerr.p, 0, 256, s));
    }
  }
  LaneBuffers b{};
  b.x = Z.d_x.as<float>();
  b.a = Z.d_a.as<_Float16>(); b.qkv = Z.d_qkv.as<_Float16>(); b.o = Z.d_o.as<_Float16>();
  b.q2 = Z.d_q2.as<_Float16>(); b.f = Z.d_f.as<_Float16>();
  b.kcache = Z.d_kc.as<_Float16>(); b.vcache = Z.d_vc.as<_Float16>();
  b.ckeys = Z.d_ck.as<_Float16>(); b.cvals = Z.d_cv.as<_Float16>();
  b.part_o = Z.d_part_o.as<float>(); b.part_ml = Z.d_part_ml.as<float>();
  b.parts = Z.d_parts.as<LogitPart>(); b.rules = Z.d_rules.as<RowRules>();
  b.lnp = Z.d_lnp.as<float2>(); b.lncnt = Z.d_lncnt.as<int>();
  b.xqk = Z.d_xqk.as<_Float16>(); b.xc = Z.d_xc.as<_Float16>();
  b.xpc = Z.d_xpc.as<float>(); b.xpml = Z.d_xpml.as<float>();
  b.enc = Z.d_enc.as<_Float16>();
  b.tokens = Z.d_tok.as<int32_t>(); b.done = Z.d_done.as<int32_t>();
  b.n_tokens = Z.d_ntok.as<int32_t>(); b.prompt = Z.d_prompt.as<int32_t>();
  b.sum_lp = Z.d_slp.as<float>(); b.nsp = Z.d_nsp.as<float>();
  b.smask = Z.d_smask.as<uint8_t>(); b.seed = Z.d_seed.as<uint32_t>(); b.itemp = Z.d_itemp.as<float>();
  b.xpairs = P.npairs() > 0 ? Z.d_xpairs.as<int4>() : nullptr;
  b.xgroups = P.ngroups() > 0 ? Z.d_xgroups.as<int>() : nullptr;
  b.roff = P.stagger() ? Z.d_roff.as<int32_t>() : nullptr;
  b.omid = Z.d_omid.as<_Float16>();
  b.segbar = Z.d_segbar.as<unsigned>(); b.segerr = Z.d_segerr.as<unsigned>();
  b.btop = Z.d_btop.as<BeamTop>(); b.bint = Z.d_bint.as<int32_t>(); b.bfin = Z.d_bfin.as<int32_t>();
  b.bfs = Z.d_bfs.as<float>();
  b.hist = P.hist() ? Z.d_hist.as<uint32_t>() : nullptr;
  b.encq = P.cross_i8 ? Z.d_encq.as<int8_t>() : nullptr;
  b.encs = P.cross_i8 ? Z.d_encs.as<float>() : nullptr;
  return b;
}

// beam search: the per-window state and the finished list inside the lane's buffers
static BeamState beam_state(const DecodePlan& P, const LaneBuffers& b, const BeamMode* beam) {
  BeamState bst{};
  if (!beam) return bst;
  const int nwin = P.nwin, B = P.B;
  int32_t* bi = b.bint;
  bst.k = beam->k; bst.length_penalty = beam->length_penalty;
  bst.nlive = bi; bst.nfin = bi + nwin; bst.wdone = bi + 2 * nwin; bst.moved = bi + 3 * nwin;
  bst.parent = bi + 4 * nwin; bst.fin_n = bi + 4 * nwin + B;
  bst.fin_tok = b.bfin; bst.fin_s = b.bfs;
  return bst;
}

// The call's inputs onto the device and the row state reset: the encoder output (copied, or
// gathered per row), the fresh rows' prompts, the offsets, seeds, temperatures, the suppress
// list and its mask, the PAIR / GROUP blocks, the counters, rule and beam state.
static void upload_inputs(janus_whisper* w, DecLane& Z, const DecodePlan& P, const LaneBuffers& b,
                          const DecodeCall& call, const BeamState& bst, hipStream_t s) {
  const janus_decode_options* opt = call.opt;
  const int B = P.B, maxlen = P.maxlen, f0 = P.f0, f1 = P.f1, V = w->cfg.n_vocab;
  const int64_t erow = (int64_t)w->cfg.n_audio_ctx * w->cfg.d_model;
  if (P.cross_i8) {
    // int8 cross-attention: the call's encoder rows quantised once, per key, from where they
    // lie (no fp16 copy); gathered rows gather the shared rows' q and s (1 byte per element)
    const int Te = w->cfg.n_audio_ctx, d = w->cfg.d_model;
    if (P.enc_rows == JANUS_ENC_ROWS_GATHERED) {
      const int n_src = call.rows->n_enc;
      Z.d_encq0.ensure((int64_t)n_src * erow);
      Z.d_encs0.ensure(sizeof(float) * (int64_t)n_src * Te);
      quant_rows_i8_launch(call.enc_in, d, Z.d_encq0.as<int8_t>(), d, Z.d_encs0.as<float>(), n_src * Te, d, s);
      for (int r = 0; r < B; ++r) {
        const int e = call.rows->enc_index[r];
        JANUS_HIP(hipMemcpyAsync(Z.d_encq.as<int8_t>() + (int64_t)r * erow, Z.d_encq0.as<int8_t>() + (int64_t)e * erow,
                                 erow, hipMemcpyDeviceToDevice, s));
        JANUS_HIP(hipMemcpyAsync(Z.d_encs.as<float>() + (int64_t)r * Te, Z.d_encs0.as<float>() + (int64_t)e * Te,
                                 sizeof(float) * Te, hipMemcpyDeviceToDevice, s));
      }
    } else {
      quant_rows_i8_launch(call.enc_in, d, Z.d_encq.as<int8_t>(), d, Z.d_encs.as<float>(), P.n_enc * Te, d, s);
    }
  } else if (P.enc_rows == JANUS_ENC_ROWS_GATHERED) {
    for (int r = 0; r < B; ++r)
      JANUS_HIP(hipMemcpyAsync(Z.d_enc.as<_Float16>() + (int64_t)r * erow, call.enc_in + (int64_t)call.rows->enc_index[r] * erow,
                               sizeof(_Float16) * erow, hipMemcpyDeviceToDevice, s));
  } else {
    JANUS_HIP(hipMemcpyAsync(Z.d_enc.p, call.enc_in, sizeof(_Float16) * (int64_t)P.n_enc * erow,
                             hipMemcpyDeviceToDevice, s));
  }
  if (P.npairs() > 0)
    JANUS_HIP(hipMemcpyAsync(Z.d_xpairs.p, P.pairs.data(), sizeof(int4) * P.npairs(), hipMemcpyHostToDevice, s));
  if (P.ngroups() > 0)
    JANUS_HIP(hipMemcpyAsync(Z.d_xgroups.p, P.groups.data(), sizeof(int) * P.groups.size(),
                             hipMemcpyHostToDevice, s));
  // synchronous uploads: the host vectors die with this call (staggered: fresh rows only)
  if (f1 > f0) {
    JANUS_HIP(hipMemcpyAsync(b.prompt + f0, P.plen.data() + f0, sizeof(int32_t) * (f1 - f0),
                             hipMemcpyHostToDevice, s));
    JANUS_HIP(hipMemcpyAsync(b.tokens + (int64_t)f0 * maxlen, P.init.data() + (size_t)f0 * maxlen,
                             sizeof(int32_t) * (size_t)(f1 - f0) * maxlen, hipMemcpyHostToDevice, s));
  }
  if (P.stagger())
    JANUS_HIP(hipMemcpyAsync(Z.d_roff.p, P.roff.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
  if (P.sampling)
    JANUS_HIP(hipMemcpyAsync(Z.d_seed.p, call.smp->seeds, sizeof(uint32_t) * B, hipMemcpyHostToDevice, s));
  if (P.row_temps)
    JANUS_HIP(hipMemcpyAsync(Z.d_itemp.p, P.itemp.data(), sizeof(float) * B, hipMemcpyHostToDevice, s));
  if (opt->n_suppress > 0)
    JANUS_HIP(hipMemcpyAsync(Z.d_supp.p, opt->suppress, sizeof(int32_t) * opt->n_suppress,
                             hipMemcpyHostToDevice, s));
  JANUS_HIP(hipStreamSynchronize(s));
  build_mask_launch(Z.d_supp.as<int32_t>(), opt->n_suppress, Z.d_smask.as<uint8_t>(), V, s);
  if (f1 > f0) {
    init_counters_launch(b.done + f0, b.sum_lp + f0, b.n_tokens + f0, Z.d_nsp.as<float>() + f0, f1 - f0, s);
    rules_init_launch(Z.d_rules.as<RowRules>() + f0, f1 - f0, s);
  }
  if (P.beam_k) beam_init_launch(bst, P.nwin, s);
  // history rules: every call starts from empty bit sets (enqueued in front of the positions,
  // so a replayed graph never sees the previous call's bits)
  if (b.hist) JANUS_HIP(hipMemsetAsync(b.hist, 0, sizeof(uint32_t) * history_words(V, w->cfg.d_model, B), s));
  JANUS_HIP(hipMemsetAsync(Z.d_lncnt.p, 0, sizeof(int) * 64, s));
}

template <class... Args> static GemmArgs dgargs(const DecodePlan& P, Args&&... args) {
  GemmArgs g = gargs(args...);
  g.msplit_n = P.msplit_n;
  g.decode_rows = true;
  return g;
}

// cross-attention keys/values, once per window (the cross-attention not absorbed)
static void project_cross_kv(janus_whisper* w, const DecodePlan& P, const LaneBuffers& b, hipStream_t s) {
  const int d = w->cfg.d_model, nl = w->cfg.dec_layers;
  const int64_t Me = (int64_t)P.B * w->cfg.n_audio_ctx;
  const _Float16* enc = b.enc;
  for (int l = 0; l < nl && !P.xabs; ++l) {
    DecLayer& L = w->dec[l];
    _Float16* ck = b.ckeys + (int64_t)l * Me * d;
    _Float16* cv = b.cvals + (int64_t)l * Me * d;
    gemm_launch(EPI_F16, dgargs(P, enc, d, L.wk_c.as<_Float16>(), d, nullptr, ck, d, (int)Me, d, d), s);
    gemm_launch(EPI_F16, dgargs(P, enc, d, L.wv_c.as<_Float16>(), d, L.bv_c, cv, d, (int)Me, d, d), s);
  }
}

// One decoder position: the launches of step(pos), in the order the plan decides. Holds the
// weights, the lane's buffers, the plan and the stream; nothing here decides a path.
struct DecodeStep : LaneBuffers {
  janus_whisper* w;
  const DecodePlan& P;
  const BeamState bst;
  hipStream_t s;
  const int d, H, Te, V, NC, nl, B, maxlen;
  const int64_t Me;
  const float scale = 0.125f;
  const float *pos_emb, *fin_g, *fin_b;
  const bool fused_ln, ln_fuse, embed_ln, lnp2, lnp3, lnp_fin, rln2, rln3, persist, layerk, xfuse;
  const DecodeRules& R;
  // the vocabulary projection's and the selectors' arguments: all but the position hold for the call
  const LogitsArgs logits = logits_args();
  const SelectArgs select = select_args();

  DecodeStep(janus_whisper* w_, const DecodePlan& plan, const LaneBuffers& buf, const BeamState& beam, hipStream_t s_)
      : LaneBuffers(buf), w(w_), P(plan), bst(beam), s(s_), d(w_->cfg.d_model), H(w_->cfg.n_heads),
        Te(w_->cfg.n_audio_ctx), V(w_->cfg.n_vocab), NC(w_->cfg.n_text_ctx), nl(w_->cfg.dec_layers),
        B(plan.B), maxlen(plan.maxlen), Me((int64_t)plan.B * w_->cfg.n_audio_ctx),
        pos_emb(w_->params.get("decoder.embed_positions.weight", (int64_t)NC * d)),
        fin_g(w_->params.get("decoder.layer_norm.weight", d)),
        fin_b(w_->params.get("decoder.layer_norm.bias", d)),
        fused_ln(plan.fused_ln), ln_fuse(plan.ln_fuse), embed_ln(plan.embed_ln),
        lnp2(plan.ln_pro_mask & 2), lnp3(plan.ln_pro_mask & 4), lnp_fin(plan.ln_pro_mask & 8),
        rln2(plan.rln && !lnp2), rln3(plan.rln && !lnp3),
        persist(plan.persist >= 1), layerk(plan.persist >= 2), xfuse(plan.persist >= 3), R(plan.R) {}

  template <class... Args> GemmArgs dgargs(Args&&... args) const { return janus::dgargs(P, args...); }
  LogitsArgs logits_args() const {
    LogitsArgs g;
    g.A = a; g.lda = d; g.W = w->tok16.as<_Float16>(); g.K = d; g.V = V; g.B = B; g.R = R;
    if (P.dec_i8) { g.Wq = w->tokq.as<int8_t>(); g.wscale = w->toks.as<float>(); }
    g.smask = smask; g.rules = rules; g.parts = parts;
    if (lnp_fin) g.lnx = x;
    g.ldx = d; g.ln_g = fin_g; g.ln_b = fin_b; g.max_blocks = P.lg_cap;
    if (P.sampling) g.seeds = seed;
    if (P.row_temps) g.row_inv_temp = itemp;
    if (P.beam_k) g.tops = btop;
    g.hist = hist; g.rep_pen = P.rep_pen;
    return g;
  }
  SelectArgs select_args() const {
    SelectArgs g;
    g.parts = parts; g.nblk = P.nblk; g.R = R; g.rules = rules; g.tokens = tokens; g.ld = maxlen;
    g.done = done; g.sum_lp = sum_lp; g.n_tok = n_tokens; g.plen = prompt; g.nsp = nsp; g.roff = roff;
    return g;
  }
  // the cross-attention launchers' arguments that hold for every layer and position
  XattnArgs xargs(int nsplit) const {
    XattnArgs xa;
    xa.qk = xqk; xa.enc = enc; xa.encq = encq; xa.escale = encs;
    xa.B = B; xa.Te = Te; xa.D = d; xa.H = H; xa.nsplit = nsplit;
    xa.part_c = xpc; xa.part_ml = xpml; xa.out = xc;
    return xa;
  }
  SkinnyLnArgs lnargs(const float* g, const float* bta, const _Float16* W, const float* bias,
                      void* C, int64_t ldc, int N, _Float16* kcp, _Float16* vcp, int pos) const {
    SkinnyLnArgs p;
    p.x = x; p.ldx = d; p.part = lnp; p.gamma = g; p.beta = bta; p.eps = 1e-5f; p.W = W; p.ldw = d;
    p.bias = bias; p.C = C; p.ldc = ldc; p.M = B; p.N = N; p.K = d;
    p.kc = kcp; p.vc = vcp; p.pos = pos; p.n_ctx = NC; p.qkv_d = d;
    return p;
  }
  // the layer's matrix JANUS_DEC_W_* (which) as the product reads it: the fp16 weights, or under
  // the int8 decoder weights their int8 copy and row scales (GemmArgs::Wq)
  GemmArgs wsel(GemmArgs g, const DecLayer& L, int which) const {
    g.W = L.w16(which).as<_Float16>();
    if (P.dec_i8) { g.W = nullptr; g.Wq = L.q8[which].as<int8_t>(); g.wscale = L.s8[which].as<float>(); }
    return g;
  }
  GemmArgs with_ln(GemmArgs g, const float* lg, const float* lb, bool on) const {
    if (on) { g.lnin_x = x; g.lnin_ldx = d; g.lnin_g = lg; g.lnin_b = lb; g.lnin_eps = 1e-5f; }
    return g;
  }
  void resid(const _Float16* A, int K, const DecLayer& L, int which, const float* bias, const float* ng,
             const float* nb) const {
    GemmArgs g = wsel(dgargs(A, K, nullptr, K, bias, x, d, B, d, K, x, d), L, which);
    if (fused_ln) g.ln_part = lnp;
    if (ln_fuse) { g.ln_g = ng; g.ln_b = nb; g.ln_out = a; g.ln_cnt = lncnt; }
    gemm_launch(EPI_RESID_F32, g, s);
  }
  void resid_ln(const _Float16* A, const DevMem& W, const float* bias, const float* ng,
                const float* nb) const {
    ResidLnArgs p;
    p.A = A; p.lda = d; p.W = W.as<_Float16>(); p.ldw = d; p.bias = bias;
    p.x = x; p.ldx = d; p.g = ng; p.b = nb; p.eps = 1e-5f; p.out = a;
    p.M = B; p.N = d; p.K = d;
    resid_ln_launch(p, s);
  }
  DecSegArgs seg_args(int l, int pos) const {
    DecLayer& L = w->dec[l];
    DecSegArgs g{};
    g.B = B; g.MT = dec_seg_mtiles(B); g.x = x;
    g.o = o; g.wo = L.wo.as<_Float16>(); g.bo = L.bo; g.ln2g = L.ln2g; g.ln2b = L.ln2b;
    g.wqk = L.wqk.as<_Float16>(); g.bqk = L.bqk.as<float>(); g.xqk = xqk;
    g.xc = xc; g.wv = L.wv_c.as<_Float16>(); g.bv = L.bv_c; g.omid = omid;
    g.woc = L.wo_c.as<_Float16>(); g.boc = L.bo_c; g.ln3g = L.ln3g; g.ln3b = L.ln3b;
    g.w1 = L.w1.as<_Float16>(); g.b1 = L.b1; g.f = f; g.w2 = L.w2.as<_Float16>(); g.b2 = L.b2;
    if (l + 1 < nl) {
      DecLayer& N = w->dec[l + 1];
      g.ln1g = N.ln1g; g.ln1b = N.ln1b; g.wqkv = N.wqkv.as<_Float16>(); g.bqkv = N.bqkv.as<float>();
      g.qkv = qkv;
      g.kc = kcache + (int64_t)(l + 1) * B * NC * d;
      g.vc = vcache + (int64_t)(l + 1) * B * NC * d;
    }
    g.pos = pos; g.n_ctx = NC; g.roff = roff;
    g.bar = segbar; g.err = segerr;
    g.prof = dec_seg_prof_target(l);
    if (layerk && l + 1 == nl && !lnp_fin) {  // the final LayerNorm as the last segment's phase
      g.fing = fin_g; g.finb = fin_b; g.fin_out = a;
    }
    if (xfuse) { g.enc = enc; g.Te = Te; }  // the cross-attention as the layer / head kernel's last phase
    return g;
  }
  // layer 0's head kernel: segment A args of layer 0 with layer 0's own LN1 / QKV / cache
  DecSegArgs head_args(int pos) const {
    DecSegArgs g = seg_args(0, pos);
    DecLayer& L0 = w->dec[0];
    g.ln1g = L0.ln1g; g.ln1b = L0.ln1b; g.wqkv = L0.wqkv.as<_Float16>(); g.bqkv = L0.bqkv.as<float>();
    g.qkv = qkv; g.kc = kcache; g.vc = vcache;
    g.fing = nullptr; g.finb = nullptr; g.fin_out = nullptr;
    return g;
  }

  // LN1 and the QKV projection of layer l (K / V rows into the cache), then the self-attention
  void qkv_self_attention(int l, int pos) const {
    DecLayer& L = w->dec[l];
    _Float16* kc = kcache + (int64_t)l * B * NC * d;
    _Float16* vc = vcache + (int64_t)l * B * NC * d;
    if (persist && (l > 0 || layerk)) {
      // q and this layer's K/V cache row came from the previous layer's segment B (layer
      // 0 with the layer kernel: from the head kernel below)
    } else if (fused_ln) {
      gemm_skinny_ln_launch(EPI_QKV, lnargs(L.ln1g, L.ln1b, L.wqkv.as<_Float16>(), L.bqkv.as<float>(),
                                            qkv, 3 * d, 3 * d, kc, vc, pos), s);
    } else {
      // layer 0's LN1 comes from the embedding kernel when embed_ln
      const bool lnp1 = (P.ln_pro_mask & 1) && !(embed_ln && l == 0);
      if (!ln_fuse && !lnp1 && !(embed_ln && l == 0))
        layernorm_launch(x, L.ln1g, L.ln1b, a, B, d, 1e-5f, s);
      if (B <= kSkinnyMaxRows) {
        GemmArgs g = with_ln(wsel(dgargs(a, d, nullptr, d, L.bqkv.as<float>(), qkv, 3 * d, B, 3 * d, d), L,
                                  JANUS_DEC_W_QKV), L.ln1g, L.ln1b, lnp1);
        g.kc = kc; g.vc = vc; g.pos = pos; g.n_ctx = NC; g.qkv_d = d;
        g.roff = roff;
        gemm_launch(EPI_QKV, g, s);
      } else {
        gemm_launch(EPI_F16, dgargs(a, d, L.wqkv.as<_Float16>(), d, L.bqkv.as<float>(), qkv, 3 * d, B, 3 * d, d), s);
        kv_store_launch(qkv, d, pos, NC, kc, vc, B, s);
      }
    }
    // (layer kernel: layers > 0 got their self-attention and segment A in the previous
    // layer's launch)
    if (!layerk)
      decode_attention_split_launch(qkv, 3 * d, kc, vc, (int64_t)NC * d, d, pos + 1, o, d, B, H, scale,
                                    part_o, part_ml, s, roff, P.max_roff);
  }

  // the rest of layer l as persistent segments (levels 1 .. 3)
  void persistent_layer(int l, int pos) const {
    const int seg_grid = P.seg_grid;
    const bool xrev = P.xrev;
    const DecSegArgs g = seg_args(l, pos);
    if (!layerk) dec_seg_a_launch(g, seg_grid, s);
    else if (l == 0) dec_head_launch(head_args(pos), seg_grid, s);
    if (!xfuse) {  // (persistent 3: the cross-attention ran as the head / layer kernel's last phase)
      XattnArgs xa = xargs(1);
      xa.rev = xrev && (l & 1);
      xattn_launch(xa, s);
    }
    if (layerk && l + 1 < nl) {
      DecLayer& N = w->dec[l + 1];
      const DecSegNext nx{N.wo.as<_Float16>(), N.bo, N.ln2g, N.ln2b, N.wqk.as<_Float16>(), N.bqk.as<float>()};
      dec_layer_launch(g, nx, seg_grid, s);
    } else {
      dec_seg_b_launch(g, seg_grid, s);
    }
  }

  // LN2, the absorbed query projection, the cross-attention over the encoder output itself
  // (one row, PAIR, GROUP or ROWS blocks), the value projection and the output projection
  void absorbed_cross_attention(int l, int pos) const {
    DecLayer& L = w->dec[l];
    const int xsplit = P.xsplit, ngroups = P.ngroups(), npairs = P.npairs(), grp_rows = P.grp_rows;
    const bool cvp = P.cvp;
    const int hd = H * d;
    if (fused_ln) {
      gemm_skinny_ln_launch(EPI_F16, lnargs(L.ln2g, L.ln2b, L.wqk.as<_Float16>(), L.bqk.as<float>(),
                                            xqk, hd, hd, nullptr, nullptr, pos), s);
    } else {
      if (!ln_fuse && !lnp2 && !rln2) layernorm_launch(x, L.ln2g, L.ln2b, a, B, d, 1e-5f, s);
      gemm_launch(EPI_F16, with_ln(wsel(dgargs(a, d, nullptr, d, L.bqk.as<float>(), xqk, hd, B, hd, d), L,
                                        JANUS_DEC_W_XQK), L.ln2g, L.ln2b, lnp2), s);
    }
    // o_h = c_h Wv_h^T + bv_h (block-diagonal over heads), then x += o Wo^T + bo; the
    // split merge and the value projection in one launch (cvp) where supported
    XattnArgs xa = xargs(xsplit);
    xa.combine = !cvp;
    if (xgroups && P.wide) {
      const int nm = P.n_main >= 0 ? P.n_main : ngroups;
      xa.groups = xgroups; xa.ngroups = nm; xa.rows_per_group = grp_rows;
      xattn_rows_launch(xa, s);
      if (ngroups > nm) {
        xa.groups = xgroups + 8 * nm; xa.ngroups = ngroups - nm; xa.rows_per_group = P.rem_rows;
        xattn_rows_launch(xa, s);
      }
      if (!cvp) xattn_combine_launch(xpc, xpml, xsplit, B, H, d, xc, s);
    } else if (xgroups) {
      xa.groups = xgroups; xa.ngroups = ngroups; xa.rows_per_group = grp_rows;
      xattn_group_launch(xa, s);
    } else {
      xa.pairs = xpairs; xa.npairs = npairs;
      if (encq) xattn_i8_launch(xa, s);   // the int8 encoder output (one row, PAIR blocks or one split)
      else xattn_launch(xa, s);
    }
    if (cvp) {
      xattn_combine_vproj_launch(xpc, xpml, xsplit, B, H, d,
                                 L.wv_c.as<_Float16>(), L.bv_c, o, d, s);
    } else {
      GemmArgs gv = wsel(dgargs(xc, hd, nullptr, d, L.bv_c, o, d, B, d, d), L, JANUS_DEC_W_XV);
      gv.a_group_cols = 64;
      gemm_launch(EPI_F16, gv, s);
    }
    if (rln3) resid_ln(o, L.wo_c, L.bo_c, L.ln3g, L.ln3b);
    else resid(o, d, L, JANUS_DEC_W_XO, L.bo_c, L.ln3g, L.ln3b);
  }

  // LN2, the query projection and the cross-attention over the per-layer projected K / V
  void projected_cross_attention(int l, int pos) const {
    DecLayer& L = w->dec[l];
    _Float16* ck = ckeys + (int64_t)l * Me * d;
    _Float16* cv = cvals + (int64_t)l * Me * d;
    if (fused_ln) {
      gemm_skinny_ln_launch(EPI_F16, lnargs(L.ln2g, L.ln2b, L.wq_c.as<_Float16>(), L.bq_c, q2, d, d,
                                            nullptr, nullptr, pos), s);
    } else {
      if (!ln_fuse && !lnp2 && !rln2) layernorm_launch(x, L.ln2g, L.ln2b, a, B, d, 1e-5f, s);
      gemm_launch(EPI_F16, with_ln(dgargs(a, d, L.wq_c.as<_Float16>(), d, L.bq_c, q2, d, B, d, d),
                                   L.ln2g, L.ln2b, lnp2), s);
    }
    decode_attention_split_launch(q2, d, ck, cv, (int64_t)Te * d, d, Te, o, d, B, H, scale, part_o,
                                  part_ml, s);
    if (rln3) resid_ln(o, L.wo_c, L.bo_c, L.ln3g, L.ln3b);
    else resid(o, d, L, JANUS_DEC_W_XO, L.bo_c, L.ln3g, L.ln3b);
  }

  // LN3, fc1 + GELU, fc2 + residual
  void mlp(int l, int pos) const {
    DecLayer& L = w->dec[l];
    if (fused_ln) {
      gemm_skinny_ln_launch(EPI_GELU_F16, lnargs(L.ln3g, L.ln3b, L.w1.as<_Float16>(), L.b1, f, 4 * d,
                                                 4 * d, nullptr, nullptr, pos), s);
    } else {
      if (!ln_fuse && !lnp3 && !rln3) layernorm_launch(x, L.ln3g, L.ln3b, a, B, d, 1e-5f, s);
      gemm_launch(EPI_GELU_F16, with_ln(wsel(dgargs(a, d, nullptr, d, L.b1, f, 4 * d, B, 4 * d, d), L,
                                             JANUS_DEC_W_FC1), L.ln3g, L.ln3b, lnp3), s);
    }
    // next LayerNorm: the following layer's LN1, or the decoder's final LN
    resid(f, 4 * d, L, JANUS_DEC_W_FC2, L.b2, l + 1 < nl ? w->dec[l + 1].ln1g : fin_g,
          l + 1 < nl ? w->dec[l + 1].ln1b : fin_b);
  }

  // the final LayerNorm, the vocabulary projection's partials, then the selection: the beam
  // step, the select + embed of the next position, or the plain select
  void tail(int pos) const {
    if (!ln_fuse && !lnp_fin && !layerk) layernorm_launch(x, fin_g, fin_b, a, B, d, 1e-5f, s);
    // history rules: the token at pos into the rows' bit sets, one launch more per position
    if (hist) history_rules_launch(tokens, maxlen, pos, prompt, P.ngram, V, logits_row_group(d), hist, B, s);
    LogitsArgs lg = logits;
    lg.pos = pos;
    logits_partial_launch(lg, s);
    SelectArgs sel = select;
    sel.pos = pos;
    if (P.beam_k) {
      beam_step_launch(sel, btop, bst, P.nwin, s);
      // the children's K / V rows of positions 0 .. pos follow their parents
      if (pos + 1 < maxlen - 1)
        beam_reorder_launch(kcache, vcache, nl, P.nwin, P.beam_k, NC, d, pos,
                            bst.parent, bst.moved, s);
      return;
    }
    if (P.fuse_se && pos + 1 < maxlen - 1)
      select_embed_launch(sel, B, s, w->tok16.as<_Float16>(), pos_emb, d, x,
                          fused_ln ? lnp : nullptr, w->dec[0].ln1g, w->dec[0].ln1b,
                          (ln_fuse || (embed_ln && !layerk)) ? a : nullptr);
    else
      select_partials_launch(sel, B, s);
  }

  // the embedding and every layer of position pos: the residual rows x before the final
  // LayerNorm (the decode call's tail, or the language head of detect_lane, comes after)
  void forward(int pos) const {
    if (!(P.fuse_se && pos >= P.sample_begin && pos > 0)) embed(pos);
    layers(pos);
  }
  // the rows' tokens at pos embedded into x (a decode call's sampled positions get theirs
  // from the previous position's select_embed instead)
  void embed(int pos) const {
    embed_launch(w->tok16.as<_Float16>(), pos_emb, tokens, maxlen, pos, d, x,
                 fused_ln ? lnp : nullptr, B, s, w->dec[0].ln1g, w->dec[0].ln1b,
                 (ln_fuse || (embed_ln && !layerk)) ? a : nullptr, roff);
  }
  void layers(int pos) const {
    for (int l = 0; l < nl; ++l) {
      DecLayer& L = w->dec[l];
      qkv_self_attention(l, pos);
      if (persist) {
        persistent_layer(l, pos);
        continue;
      }
      if (rln2) resid_ln(o, L.wo, L.bo, L.ln2g, L.ln2b);
      else resid(o, d, L, JANUS_DEC_W_O, L.bo, L.ln2g, L.ln2b);
      if (P.xabs) absorbed_cross_attention(l, pos);
      else projected_cross_attention(l, pos);
      mlp(l, pos);
    }
  }

  void operator()(int pos) const {
    forward(pos);
    if (pos + 1 < P.sample_begin) return;  // still inside the prompt
    tail(pos);
  }
};

// The positions in chunks: each chunk one captured graph (cached on the lane under the
// plan's and the buffers' key), the early exit polled between chunks.
static void run_positions(DecLane& Z, const DecodePlan& P, const LaneBuffers& b, const DecodeStep& step,
                          hipStream_t s) {
  const int B = P.B, chunk = P.chunk, steps = P.steps;
  // every device pointer a captured kernel touches, plus the shape: the graph cache key
  std::vector<int64_t> base_key;
  P.append_key(base_key);
  b.append_key(base_key);
  std::vector<int32_t> h_done(B);
  if (Z.graphs.size() > 512) Z.drop_graphs();
  for (int p0 = 0; p0 < steps; p0 += chunk) {
    const int n = std::min(chunk, steps - p0);
    Z.last_positions += n;
    if (P.use_graph) {
      std::vector<int64_t> key = base_key;
      key.push_back(p0);
      key.push_back(n);
      auto it = Z.graphs.find(key);
      if (it == Z.graphs.end()) {
        hipGraph_t g;
        JANUS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
          for (int pos = p0; pos < p0 + n; ++pos) step(pos);
        } catch (...) {
          hipGraph_t dead;
          (void)hipStreamEndCapture(s, &dead);
          if (dead) (void)hipGraphDestroy(dead);
          throw;
        }
        JANUS_HIP(hipStreamEndCapture(s, &g));
        size_t nodes = 0;
        JANUS_HIP(hipGraphGetNodes(g, nullptr, &nodes));
        hipGraphExec_t ge;
        JANUS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        JANUS_HIP(hipGraphDestroy(g));
        it = Z.graphs.emplace(key, ge).first;
        Z.graph_nodes[key] = nodes;
      }
      JANUS_HIP(hipGraphLaunch(it->second, s));
      Z.last_launches += (int64_t)Z.graph_nodes[key];
    } else {
      for (int pos = p0; pos < p0 + n; ++pos) step(pos);
    }
    if (P.check_every > 0 && p0 + n >= P.sample_begin) {
      JANUS_HIP(hipMemcpyAsync(h_done.data(), b.done, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
      JANUS_HIP(hipStreamSynchronize(s));
      bool all = true;
      for (int r = 0; r < B; ++r) all = all && h_done[r];
      if (all) break;  // remaining positions keep -1; callers stop at the first eot
    }
  }
}

// After the positions: the persistent segments' barrier-timeout flag, where the rows stand,
// and the outputs (beam search: every window's winner).
static void finish(DecLane& Z, const DecodePlan& P, const LaneBuffers& b, const DecodeCall& call,
                   const BeamState& bst, hipStream_t s) {
  const int B = P.B, maxlen = P.maxlen;
  const bool persist = P.persist > 0;
  if (persist && P.check_every <= 0) {   // the check deferred: the call does not wait
    if (!Z.h_segerr) JANUS_HIP(hipHostMalloc((void**)&Z.h_segerr, sizeof(uint32_t), hipHostMallocDefault));
    if (!Z.ev_segerr) JANUS_HIP(hipEventCreateWithFlags(&Z.ev_segerr, hipEventDisableTiming));
    JANUS_HIP(hipMemcpyAsync(Z.h_segerr, Z.d_segerr.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    JANUS_HIP(hipEventRecord(Z.ev_segerr, s));
    Z.segerr_pending = true;
  } else if (persist) {  // a segment whose grid never became co-resident gave up at a barrier
    uint32_t herr = 0;
    JANUS_HIP(hipMemcpyAsync(&herr, Z.d_segerr.p, sizeof(herr), hipMemcpyDeviceToHost, s));
    JANUS_HIP(hipStreamSynchronize(s));
    if (herr) {
      JANUS_HIP(hipMemsetAsync(Z.d_segbar.p, 0, sizeof(unsigned) * 256, s));
      JANUS_HIP(hipMemsetAsync(Z.d_segerr.p, 0, 256, s));
      JANUS_HIP(hipStreamSynchronize(s));
      throw Error("decode: a persistent decoder segment timed out at a grid barrier (grid not co-resident)");
    }
  }
  // every row ran Z.last_positions positions from its offset (the early exit stops all rows
  // together); janus_whisper_decode_stand reports it, stagger plans continue from there
  Z.stand.assign(B, 0);
  for (int r = 0; r < B; ++r) Z.stand[r] = (P.stagger() ? P.roff[r] : 0) + Z.last_positions;
  Z.stand_maxlen = maxlen;
  if (P.beam_k) {  // one output row per window: its winner
    Z.stand.clear();  // nothing here is a row a staggered call could continue
    beam_finish_launch(bst, P.R, b.tokens, maxlen, b.sum_lp, b.n_tokens, Z.d_prompt.as<int32_t>(), Z.d_nsp.as<float>(),
                       P.nwin, call.tokens_out, call.n_tokens_out, call.sum_lp_out, call.nsp_out, s);
    return;
  }
  JANUS_HIP(hipMemcpyAsync(call.tokens_out, b.tokens, sizeof(int32_t) * (int64_t)B * maxlen,
                           hipMemcpyDeviceToDevice, s));
  JANUS_HIP(hipMemcpyAsync(call.n_tokens_out, b.n_tokens, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
  JANUS_HIP(hipMemcpyAsync(call.sum_lp_out, b.sum_lp, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
  if (call.nsp_out)
    JANUS_HIP(hipMemcpyAsync(call.nsp_out, Z.d_nsp.p, sizeof(float) * B, hipMemcpyDeviceToDevice, s));
}

// One decode call on one lane (greedy, sampled or beam search): plan, then run.
static void decode_lane(janus_whisper* w, DecLane& Z, const DecodeCall& call, int B, hipStream_t s,
                        LaneLatch* latch) {
  LaneArrival arrival(latch);   // (first: a lane that throws below must still arrive)
  lane_check(Z);   // the previous non-polling call's flag first
  const DecodePlan P = plan_decode(w->cfg, *call.opt, call.rows, call.smp, call.beam, B, stream_cu_count(s),
                                   latch != nullptr, LaneStand{&Z.stand, Z.stand_maxlen},
                                   SegDevice{dec_seg_grid, dec_seg_resident}, w->cross_compute, w->dec_compute);
  // until this call completes, nothing may be continued (a failed call leaves stand empty)
  Z.stand.clear();
  const LaneBuffers b = ensure_buffers(w, Z, P, call.opt->n_suppress, s);
  const BeamState bst = beam_state(P, b, call.beam);
  upload_inputs(w, Z, P, b, call, bst, s);
  project_cross_kv(w, P, b, s);
  const DecodeStep step(w, P, b, bst, s);
  arrival.now();  // all lanes' allocations done: captures may start
  Z.last_positions = 0;
  Z.last_launches = 0;
  Z.last_enc_rows = P.enc_rows;
  Z.last_persist = P.persist;
  Z.last_cross = P.cross_i8 ? JANUS_CROSS_COMPUTE_INT8 : JANUS_CROSS_COMPUTE_F16;
  Z.last_weights = P.dec_i8 ? JANUS_DEC_COMPUTE_INT8 : JANUS_DEC_COMPUTE_F16;
  run_positions(Z, P, b, step, s);
  finish(Z, P, b, call, bst, s);
}

// Language identification of up to kLangRows windows (janus_whisper_detect_language): the
// decode call's own machinery — a plan with the one-token prompt [sot] and one position (so
// the prepared weights, the cross-attention path and the launch geometry are the decode
// call's), run on the context's language lane — with the tail replaced by the language head
// (langid.hip) over the position's residual rows. Launched directly: one position, once.
constexpr int kLangRows = 64;
static void detect_lane(janus_whisper* w, DecLane& Z, const _Float16* enc, int B, int sot, int lang_begin,
                        int n_lang, float* probs, int32_t* best, hipStream_t s) {
  janus_decode_options opt{};
  const int32_t prompt[1] = {sot};
  opt.prompt = prompt; opt.prompt_len = 1; opt.max_length = 2;
  opt.eot = -1; opt.blank_token = -1; opt.timestamp_begin = -1; opt.no_timestamps = -1;
  opt.max_initial_timestamp_index = -1;
  opt.check_every = 0;
  opt.path_flags = JANUS_DEC_PATH_NO_GRAPH;
  const DecodePlan P = plan_decode(w->cfg, opt, nullptr, nullptr, nullptr, B, stream_cu_count(s), false,
                                   LaneStand{&Z.stand, Z.stand_maxlen}, SegDevice{dec_seg_grid, dec_seg_resident});
  Z.stand.clear();
  const LaneBuffers b = ensure_buffers(w, Z, P, 0, s);
  const BeamState bst{};
  const DecodeCall call{enc, &opt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  upload_inputs(w, Z, P, b, call, bst, s);
  project_cross_kv(w, P, b, s);
  const DecodeStep step(w, P, b, bst, s);
  step.forward(0);
  lang_head_launch(b.x, step.fin_g, step.fin_b, w->tok16.as<_Float16>(), w->cfg.d_model, w->cfg.n_vocab,
                   lang_begin, n_lang, B, probs, best, s);
}

// The residual rows of forced tokens (janus_whisper_decode_hidden, test entry): a decode
// call's plan, buffers, uploads and cross K/V, then every position's embedding and layers
// launched directly and x copied out after each — no tail, so no token is selected and the
// embedding of every position comes from the embedding kernel.
static void hidden_lane(janus_whisper* w, DecLane& Z, const DecodeCall& call, int B, float* x_out,
                        int x_positions, _Float16* kc_out, _Float16* vc_out, char* text, int text_cap,
                        hipStream_t s) {
  lane_check(Z);
  const DecodePlan P = plan_decode(w->cfg, *call.opt, call.rows, nullptr, nullptr, B, stream_cu_count(s), false,
                                   LaneStand{&Z.stand, Z.stand_maxlen}, SegDevice{dec_seg_grid, dec_seg_resident},
                                   w->cross_compute, w->dec_compute);
  JANUS_CHECK(P.steps <= x_positions, "decode_hidden: x_out holds fewer positions than the call runs");
  const std::string desc = P.describe();
  JANUS_CHECK(text && (int64_t)desc.size() < text_cap, "decode_hidden: plan_text too small");
  std::memcpy(text, desc.c_str(), desc.size() + 1);
  Z.stand.clear();
  const LaneBuffers b = ensure_buffers(w, Z, P, call.opt->n_suppress, s);
  const BeamState bst{};
  upload_inputs(w, Z, P, b, call, bst, s);
  // the forced tokens of every row: a continuing row's positions of this call too
  JANUS_HIP(hipMemcpyAsync(b.tokens, P.init.data(), sizeof(int32_t) * (size_t)B * P.maxlen,
                           hipMemcpyHostToDevice, s));
  project_cross_kv(w, P, b, s);
  const DecodeStep step(w, P, b, bst, s);
  const int64_t xrow = (int64_t)B * w->cfg.d_model;
  for (int pos = 0; pos < P.steps; ++pos) {
    step.embed(pos);
    step.layers(pos);
    JANUS_HIP(hipMemcpyAsync(x_out + pos * xrow, b.x, sizeof(float) * xrow, hipMemcpyDeviceToDevice, s));
  }
  const int64_t cache = (int64_t)w->cfg.dec_layers * B * w->cfg.n_text_ctx * w->cfg.d_model;
  if (kc_out) JANUS_HIP(hipMemcpyAsync(kc_out, b.kcache, sizeof(_Float16) * cache, hipMemcpyDeviceToDevice, s));
  if (vc_out) JANUS_HIP(hipMemcpyAsync(vc_out, b.vcache, sizeof(_Float16) * cache, hipMemcpyDeviceToDevice, s));
  uint32_t herr = 0;   // a segment that gave up at a barrier: an error, not data (as finish)
  if (P.persist > 0)
    JANUS_HIP(hipMemcpyAsync(&herr, Z.d_segerr.p, sizeof(herr), hipMemcpyDeviceToHost, s));
  JANUS_HIP(hipStreamSynchronize(s));   // (P.init and herr die with this call)
  if (herr) {
    JANUS_HIP(hipMemsetAsync(Z.d_segbar.p, 0, sizeof(unsigned) * 256, s));
    JANUS_HIP(hipMemsetAsync(Z.d_segerr.p, 0, 256, s));
    JANUS_HIP(hipStreamSynchronize(s));
    throw Error("decode: a persistent decoder segment timed out at a grid barrier (grid not co-resident)");
  }
  Z.last_positions = P.steps;
  Z.last_launches = 0;
  Z.last_enc_rows = P.enc_rows;
  Z.last_persist = P.persist;
  Z.last_cross = P.cross_i8 ? JANUS_CROSS_COMPUTE_INT8 : JANUS_CROSS_COMPUTE_F16;
  Z.last_weights = P.dec_i8 ? JANUS_DEC_COMPUTE_INT8 : JANUS_DEC_COMPUTE_F16;
  Z.stand.assign(B, 0);
  for (int r = 0; r < B; ++r) Z.stand[r] = (P.stagger() ? P.roff[r] : 0) + P.steps;
  Z.stand_maxlen = P.maxlen;
}

}  // namespace janus

using namespace janus;

extern "C" int janus_whisper_decode_hidden(janus_whisper* w, const uint16_t* enc, int batch,
                                           const janus_decode_options* opt, const janus_decode_rows* rows,
                                           float* x_out, int x_positions, uint16_t* kc_out, uint16_t* vc_out,
                                           char* plan_text, int plan_cap, void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && enc && opt && rows && x_out && plan_text, "null argument");
    JANUS_CHECK(batch >= 1, "decode_hidden: batch must be >= 1");
    JANUS_CHECK(rows->prompts && rows->prompt_lens, "decode_hidden: the forced tokens are the per-row prompts");
    const int n = rows->prompt_lens[0];
    for (int b = 0; b < batch; ++b)
      JANUS_CHECK(rows->prompt_lens[b] == n, "decode_hidden: every row's prompt must have the same length");
    JANUS_CHECK(opt->state_slot >= 0 && opt->state_slot < 8, "decode: state_slot must be 0 .. 7");
    std::lock_guard<std::mutex> lk(w->mu);
    hipStream_t s = (hipStream_t)stream;
    prepare(w, s);
    if (w->dec_compute == JANUS_DEC_COMPUTE_INT8) prepare_dec_i8(w, s);
    janus_decode_options o = *opt;
    o.max_length = n + 1;   // every position is inside the prompt: nothing is sampled
    while ((int)w->lanes.size() <= o.state_slot) w->lanes.emplace_back(new DecLane());
    w->last_slot = o.state_slot;
    hidden_lane(w, *w->lanes[o.state_slot],
                DecodeCall{reinterpret_cast<const _Float16*>(enc), &o, rows, nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr},
                batch, x_out, x_positions, reinterpret_cast<_Float16*>(kc_out), reinterpret_cast<_Float16*>(vc_out),
                plan_text, plan_cap, s);
  });
}

extern "C" int janus_whisper_detect_language(janus_whisper* w, const uint16_t* enc, int batch, int sot_token,
                                             int lang_begin, int n_lang, float* probs, int32_t* best,
                                             void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && enc && probs && best, "null argument");
    JANUS_CHECK(batch >= 1, "detect_language: batch must be >= 1");
    const int V = w->cfg.n_vocab;
    JANUS_CHECK(sot_token >= 0 && sot_token < V, "detect_language: sot_token out of range");
    JANUS_CHECK(n_lang >= 1 && n_lang <= 128 && lang_begin >= 0 && lang_begin + n_lang <= V,
                "detect_language: need 1 <= n_lang <= 128 and lang_begin + n_lang <= n_vocab");
    JANUS_CHECK(w->cfg.d_model % 8 == 0, "detect_language: d_model % 8 != 0");
    std::lock_guard<std::mutex> lk(w->mu);
    hipStream_t s = (hipStream_t)stream;
    prepare(w, s);
    if (!w->lang_lane) w->lang_lane.reset(new DecLane());
    const _Float16* e = reinterpret_cast<const _Float16*>(enc);
    const int64_t erow = (int64_t)w->cfg.n_audio_ctx * w->cfg.d_model;
    // larger batches in chunks of kLangRows windows, as the decode entry's lanes slice a batch
    for (int b0 = 0; b0 < batch; b0 += kLangRows) {
      const int n = std::min(kLangRows, batch - b0);
      detect_lane(w, *w->lang_lane, e + b0 * erow, n, sot_token, lang_begin, n_lang,
                  probs + (int64_t)b0 * n_lang, best + b0, s);
    }
  });
}

extern "C" int janus_whisper_decode_greedy(janus_whisper* w, const uint16_t* enc, int batch,
                                           const janus_decode_options* opt, int32_t* tokens,
                                           int32_t* n_tokens, float* sum_logprob, void* stream) {
  return janus_whisper_decode_greedy_ex(w, enc, batch, opt, nullptr, tokens, n_tokens, sum_logprob,
                                        nullptr, stream);
}

static int decode_entry(janus_whisper* w, const uint16_t* enc, int batch,
                        const janus_decode_options* opt, const janus_decode_rows* rows,
                        int32_t* tokens, int32_t* n_tokens, float* sum_logprob,
                        float* no_speech_prob, void* stream, const DecodeSampling* smp,
                        const BeamMode* beam = nullptr);

extern "C" int janus_whisper_decode_greedy_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                              const janus_decode_options* opt,
                                              const janus_decode_rows* rows, int32_t* tokens,
                                              int32_t* n_tokens, float* sum_logprob,
                                              float* no_speech_prob, void* stream) {
  return decode_entry(w, enc, batch, opt, rows, tokens, n_tokens, sum_logprob, no_speech_prob, stream,
                      nullptr);
}

extern "C" int janus_whisper_decode_sample_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                              const janus_decode_options* opt,
                                              const janus_decode_rows* rows, float temperature,
                                              const uint32_t* seeds, int32_t* tokens,
                                              int32_t* n_tokens, float* sum_logprob,
                                              float* no_speech_prob, void* stream) {
  if (!(temperature > 0.f) || !seeds) {
    set_error("decode_sample: temperature must be > 0 and seeds non-null");
    return -1;
  }
  const DecodeSampling smp{temperature, seeds};
  return decode_entry(w, enc, batch, opt, rows, tokens, n_tokens, sum_logprob, no_speech_prob, stream,
                      &smp);
}

extern "C" int janus_whisper_decode_sample_rows_ex(janus_whisper* w, const uint16_t* enc, int batch,
                                                   const janus_decode_options* opt,
                                                   const janus_decode_rows* rows, const float* temperatures,
                                                   const uint32_t* seeds, int32_t* tokens,
                                                   int32_t* n_tokens, float* sum_logprob,
                                                   float* no_speech_prob, void* stream) {
  if (!temperatures || !seeds || batch <= 0) {
    set_error("decode_sample_rows: temperatures and seeds must be non-null");
    return -1;
  }
  for (int b = 0; b < batch; ++b)
    if (!(temperatures[b] >= 0.f)) {
      set_error("decode_sample_rows: every temperature must be >= 0");
      return -1;
    }
  const DecodeSampling smp{1.0f, seeds, temperatures};
  return decode_entry(w, enc, batch, opt, rows, tokens, n_tokens, sum_logprob, no_speech_prob, stream,
                      &smp);
}

extern "C" int janus_whisper_decode_beam_ex(janus_whisper* w, const uint16_t* enc, int n_windows,
                                            const janus_decode_options* opt, const janus_decode_rows* rows,
                                            int beam_size, float length_penalty, int32_t* tokens,
                                            int32_t* n_tokens, float* sum_logprob, float* no_speech_prob,
                                            void* stream) {
  return guarded([&] {
    JANUS_CHECK(w && enc && opt && tokens && n_tokens && sum_logprob, "null argument");
    JANUS_CHECK(n_windows >= 1, "decode_beam: n_windows must be >= 1");
    JANUS_CHECK(beam_size >= 1 && beam_size <= kBeamMax, "decode_beam: beam_size must be 1 .. 8");
    JANUS_CHECK(length_penalty > 0.f, "decode_beam: length_penalty must be > 0");
    JANUS_CHECK((int64_t)n_windows * beam_size <= kSkinnyMaxRows,
                "decode_beam: windows x beam_size must be <= 512 rows");
    JANUS_CHECK(!(rows && rows->pos_offset), "decode_beam: staggered rows (pos_offset) are not supported");
    JANUS_CHECK(!(rows && rows->enc_index), "decode_beam: enc_index is built by the call (one encoder row per window)");
    const int k = beam_size, B = n_windows * k;
    // the window's prompt on each of its k rows, all of them on the window's encoder row
    const bool per_row = rows && rows->prompts;
    JANUS_CHECK(per_row || (opt->prompt && opt->prompt_len >= 1), "decode: missing prompt");
    JANUS_CHECK(!per_row || (rows->prompt_lens && rows->stride >= 1), "decode: per-row prompts need lengths and a stride");
    const int stride = per_row ? rows->stride : opt->prompt_len;
    std::vector<int32_t> prompts((size_t)B * stride, 0), plens(B), eidx(B);
    for (int b = 0; b < B; ++b) {
      const int wi = b / k;
      eidx[b] = wi;
      plens[b] = per_row ? rows->prompt_lens[wi] : opt->prompt_len;
      JANUS_CHECK(plens[b] >= 1 && plens[b] <= stride, "decode: per-row prompt length out of range");
      const int32_t* src = per_row ? rows->prompts + (size_t)wi * stride : opt->prompt;
      std::copy(src, src + plens[b], prompts.begin() + (size_t)b * stride);
    }
    janus_decode_rows br{};
    br.prompts = prompts.data(); br.prompt_lens = plens.data(); br.stride = stride;
    br.no_speech_token = rows ? rows->no_speech_token : -1;
    br.no_speech_back = rows ? rows->no_speech_back : 0;
    br.enc_index = eidx.data(); br.n_enc = n_windows;
    const BeamMode bm{k, length_penalty};
    // (shared encoder rows: one lane; a null stream gets the lane's own, as every decode)
    const int rc = decode_entry(w, enc, B, opt, &br, tokens, n_tokens, sum_logprob, no_speech_prob, stream,
                                nullptr, &bm);
    JANUS_CHECK(rc == 0, janus_last_error());
  });
}

extern "C" int janus_whisper_decode_stand_slot(janus_whisper* w, int slot, int32_t* stand, int batch) {
  return guarded([&] {
    JANUS_CHECK(w && stand, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    JANUS_CHECK(slot >= 0 && slot < (int)w->lanes.size() && (int)w->lanes[slot]->stand.size() == batch,
                "decode_stand: no completed decode of this batch size in this slot");
    std::copy(w->lanes[slot]->stand.begin(), w->lanes[slot]->stand.end(), stand);
  });
}

extern "C" int janus_whisper_decode_check(janus_whisper* w, int slot) {
  return guarded([&] {
    JANUS_CHECK(w, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    JANUS_CHECK(slot >= 0 && slot < 8, "decode_check: slot must be 0 .. 7");
    if (slot < (int)w->lanes.size()) lane_check(*w->lanes[slot]);
  });
}

extern "C" int janus_whisper_decode_stand(janus_whisper* w, int32_t* stand, int batch) {
  return janus_whisper_decode_stand_slot(w, 0, stand, batch);
}

extern "C" int janus_whisper_decode_info(janus_whisper* w, int32_t* positions, int64_t* launches) {
  return guarded([&] {
    JANUS_CHECK(w && positions && launches, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    const int sl = w->last_slot < (int)w->lanes.size() ? w->last_slot : 0;
    *positions = w->lanes.empty() ? 0 : w->lanes[sl]->last_positions;
    *launches = w->lanes.empty() ? 0 : w->lanes[sl]->last_launches;
  });
}

extern "C" int janus_whisper_decode_path(janus_whisper* w, int32_t* enc_rows, int32_t* persistent) {
  return guarded([&] {
    JANUS_CHECK(w && enc_rows && persistent, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    const int sl = w->last_slot < (int)w->lanes.size() ? w->last_slot : 0;
    *enc_rows = w->lanes.empty() ? JANUS_ENC_ROWS_OWN : w->lanes[sl]->last_enc_rows;
    *persistent = w->lanes.empty() ? 0 : w->lanes[sl]->last_persist;
  });
}

extern "C" int janus_whisper_decode_cross(janus_whisper* w, int32_t* mode) {
  return guarded([&] {
    JANUS_CHECK(w && mode, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    const int sl = w->last_slot < (int)w->lanes.size() ? w->last_slot : 0;
    *mode = w->lanes.empty() ? JANUS_CROSS_COMPUTE_F16 : w->lanes[sl]->last_cross;
  });
}

extern "C" int janus_whisper_decode_weights(janus_whisper* w, int32_t* mode) {
  return guarded([&] {
    JANUS_CHECK(w && mode, "null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    const int sl = w->last_slot < (int)w->lanes.size() ? w->last_slot : 0;
    *mode = w->lanes.empty() ? JANUS_DEC_COMPUTE_F16 : w->lanes[sl]->last_weights;
  });
}

static int decode_entry(janus_whisper* w, const uint16_t* enc, int batch,
                        const janus_decode_options* opt, const janus_decode_rows* rows,
                        int32_t* tokens, int32_t* n_tokens, float* sum_logprob,
                        float* no_speech_prob, void* stream, const DecodeSampling* smp,
                        const BeamMode* beam) {
  return guarded([&] {
    JANUS_CHECK(w && enc && opt && tokens && n_tokens && sum_logprob, "null argument");
    JANUS_CHECK(batch >= 1, "decode: batch must be >= 1");
    std::lock_guard<std::mutex> lk(w->mu);
    hipStream_t s = (hipStream_t)stream;
    prepare(w, s);
    if (w->dec_compute == JANUS_DEC_COMPUTE_INT8 && !beam) prepare_dec_i8(w, s);
    const _Float16* e = reinterpret_cast<const _Float16*>(enc);
    // lanes: janus_decode_options.lanes (default 1). Two half-batch lanes measured slower at B = 64
    // (428.7 vs 419.6 ms per bench step): the skinny projections are weight-stream
    // launches, so each lane re-streams every weight matrix, and the cross-attention
    // already saturates HBM.
    int nlanes = opt->lanes > 0 ? opt->lanes : 1;
    nlanes = std::max(1, std::min(nlanes, std::min(batch, 8)));
    // shared encoder rows / staggered rows: one lane holds them all (and its slots' state)
    if (rows && (rows->enc_index || rows->pos_offset)) nlanes = 1;
    // a state slot other than 0 (janus_decode_options.state_slot) is one lane of its own
    JANUS_CHECK(opt->state_slot >= 0 && opt->state_slot < 8, "decode: state_slot must be 0 .. 7");
    const int slot = opt->state_slot;
    if (slot > 0) nlanes = 1;
    // storage: state slots 0..7 are lanes[0..7]; the extra workers of a multi-lane call
    // (lanes 1..7) live in lanes[8..14], so they never overwrite a slot's KV caches,
    // tokens, graphs or stand (the staggered step's fallback keeps state in slot 1)
    auto lane_of = [](int i) { return i == 0 ? 0 : 7 + i; };
    const int need = std::max(slot + 1, nlanes > 1 ? lane_of(nlanes - 1) + 1 : 1);
    while ((int)w->lanes.size() < need) w->lanes.emplace_back(new DecLane());
    w->last_slot = slot;
    if (nlanes == 1 && (s != nullptr || slot > 0)) {
      JANUS_CHECK(s != nullptr, "decode: a state slot > 0 needs a non-null stream");
      decode_lane(w, *w->lanes[slot],
                  DecodeCall{e, opt, rows, smp, beam, tokens, n_tokens, sum_logprob, no_speech_prob}, batch, s,
                  nullptr);
      return;
    }
    // the null stream cannot be captured, and lanes run concurrently: each lane gets its
    // own stream (the caller's priority), forked from and joined back into the caller's
    int prio = 0;
    JANUS_HIP(hipStreamGetPriority(s, &prio));
    if (!w->ev_in) JANUS_HIP(hipEventCreateWithFlags(&w->ev_in, hipEventDisableTiming));
    JANUS_HIP(hipEventRecord(w->ev_in, s));
    // a caller on a CU-masked stream (the overlapped step's decoder partition) gets lanes
    // on the same CUs
    std::vector<uint32_t> mask(16, 0xffffffffu);
    bool masked = false;
    if (s && hipExtStreamGetCUMask(s, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
      int ncu = 0;
      JANUS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
      for (int c = 0; c < ncu && c < 32 * (int)mask.size(); ++c)
        if (!((mask[c / 32] >> (c % 32)) & 1u)) masked = true;
    }
    for (int i = 0; i < nlanes; ++i) {
      DecLane& Z = *w->lanes[lane_of(i)];
      if (Z.stream && Z.stream_mask != (masked ? mask : std::vector<uint32_t>())) {
        JANUS_HIP(hipStreamSynchronize(Z.stream));
        JANUS_HIP(hipStreamDestroy(Z.stream));
        Z.stream = nullptr;
        Z.drop_graphs();
      }
      if (!Z.stream) {
        if (masked)
          JANUS_HIP(hipExtStreamCreateWithCUMask(&Z.stream, (uint32_t)mask.size(), mask.data()));
        else
          JANUS_HIP(hipStreamCreateWithPriority(&Z.stream, hipStreamNonBlocking, prio));
        Z.stream_mask = masked ? mask : std::vector<uint32_t>();
        if (!Z.ev_done) JANUS_HIP(hipEventCreateWithFlags(&Z.ev_done, hipEventDisableTiming));
      }
      JANUS_HIP(hipStreamWaitEvent(Z.stream, w->ev_in, 0));
    }
    const int maxlen = opt->max_length;
    LaneLatch latch;
    latch.left = nlanes;
    std::vector<std::string> errs(nlanes);
    int dev = 0;
    JANUS_HIP(hipGetDevice(&dev));
    auto run = [&](int i) {
      const int b0 = (int)((int64_t)batch * i / nlanes), b1 = (int)((int64_t)batch * (i + 1) / nlanes);
      DecLane& Z = *w->lanes[lane_of(i)];
      try {
        JANUS_HIP(hipSetDevice(dev));  // a fresh host thread starts on device 0
        janus_decode_rows sub{};
        if (rows) {
          sub = *rows;
          if (rows->prompts) {
            sub.prompts = rows->prompts + (int64_t)b0 * rows->stride;
            sub.prompt_lens = rows->prompt_lens + b0;
          }
        }
        DecodeSampling ssub{};
        if (smp) ssub = DecodeSampling{smp->temperature, smp->seeds + b0, smp->temps ? smp->temps + b0 : nullptr};
        decode_lane(w, Z,
                    DecodeCall{e + (int64_t)b0 * w->cfg.n_audio_ctx * w->cfg.d_model, opt,
                               rows ? &sub : nullptr, smp ? &ssub : nullptr, beam, tokens + (int64_t)b0 * maxlen,
                               n_tokens + b0, sum_logprob + b0, no_speech_prob ? no_speech_prob + b0 : nullptr},
                    b1 - b0, Z.stream, nlanes > 1 ? &latch : nullptr);
      } catch (const std::exception& ex) {
        errs[i] = ex.what();
      } catch (...) {
        errs[i] = "unknown error";
      }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < nlanes; ++i) th.emplace_back(run, i);
    run(0);
    for (auto& t : th) t.join();
    for (int i = 0; i < nlanes; ++i) {
      DecLane& Z = *w->lanes[lane_of(i)];
      JANUS_HIP(hipEventRecord(Z.ev_done, Z.stream));
      JANUS_HIP(hipStreamWaitEvent(s, Z.ev_done, 0));
    }
    for (int i = 0; i < nlanes; ++i)
      JANUS_CHECK(errs[i].empty(), "decode lane " + std::to_string(i) + ": " + errs[i]);
  });
}

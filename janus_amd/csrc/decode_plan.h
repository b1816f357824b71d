// The plan of one decode call on one lane: every check of the call's arguments and every
// decision about the path its positions take, made once, as data, before the lane or the
// stream is touched (plan_decode). Host only: no device work, no HIP header — what needs the
// device (the CU count, the persistent grids' occupancy) is passed in.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "decode_shapes.h"
#include "../../include/janus.h"

namespace janus {

// Sampling (faster-whisper's temperature fallback, CTranslate2 generate(sampling_temperature=
// T, sampling_topk=0)): temperature > 0 draws each token from softmax(filtered logits / T)
// by Gumbel-max with per-row counter-based noise (seeds [host] uint32 [B]); null = greedy.
struct DecodeSampling {
  float temperature;
  const uint32_t* seeds;
  const float* temps = nullptr;   // host [B], per-row temperatures (overrides temperature)
};

// Beam search (janus_whisper_decode_beam_ex): the call's rows are windows x k, row w * k + j
// beam j of window w (the entry builds enc_index and the per-row prompts); the selection is
// the beam step + the KV reorder, and the outputs are one row per window.
struct BeamMode {
  int k;
  float length_penalty;
};

// Where the lane's row slots stand after its last call (DecLane::stand / stand_maxlen)
struct LaneStand {
  const std::vector<int32_t>* stand;
  int maxlen;
};

// What the persistent segments ask the device (dec_persist.h): the resident grid for B rows
// on `cus` CUs (its two-blocks-per-CU form asks for occupancy) and whether a grid is
// co-resident. Callables, so a test answers them without a device.
struct SegDevice {
  std::function<int(int B, int cus, bool two_per_cu)> grid;   // dec_seg_grid
  std::function<bool(int grid, int cus)> resident;            // dec_seg_resident
};

// decoder rows b0 and b1 (b1 < 0: none) attending to encoder row e (xattn_launch's int4)
struct XPair {
  int32_t b0, b1, e, pad;
};
static_assert(sizeof(XPair) == 16, "XPair is the device's int4");

// a scalar plan field as a word of the graph cache key (a float by its bits)
inline int64_t key_word(float v) {
  uint32_t u;
  std::memcpy(&u, &v, sizeof(u));
  return (int64_t)u;
}
inline int64_t key_word(int v) { return v; }
inline int64_t key_word(bool v) { return v; }

// the graph key's word of a call with the int8 cross-attention ("xi8" above any 32-bit field)
constexpr int64_t kCrossI8KeyWord = (int64_t)0x786938 << 32;
// likewise of a call with the int8 decoder weights ("wi8")
constexpr int64_t kDecI8KeyWord = (int64_t)0x776938 << 32;

struct DecodePlan {
  // ---- shape and counts
  int B = 0, maxlen = 0;
  int steps = 0;            // positions every row runs from its own offset
  int chunk = 0;            // positions per captured graph (and per early-exit poll)
  int check_every = 0;      // janus_decode_options.check_every (0: no early-exit polling)
  int sample_begin = 0;     // index of the first sampled token (earliest row)
  int f0 = 0, f1 = 0;       // the fresh rows [f0, f1) (not staggered: every row)
  int max_roff = 0;
  int nsp_back = 0;         // janus_decode_rows.no_speech_back
  int nwin = 0, beam_k = 0; // beam search: windows and beams per window (0: off)
  // ---- paths
  int enc_rows = JANUS_ENC_ROWS_OWN;   // how the rows reach their encoder output
  int n_enc = 0;            // rows of the lane's encoder buffer (read in place: the shared rows)
  bool wide = false;        // the 12-head family at d = 768 (not H <= 8, d <= 512)
  bool xabs = false;        // absorbed cross-attention
  int xsplit = 0;
  bool cvp = false;
  bool fused_ln = false, ln_fuse = false;
  int ln_pro_mask = 0;
  bool embed_ln = false, rln = false, fuse_se = false;
  int seg_grid = 0;
  int persist = 0;          // persistent level run, 0 .. 3 (0: the launch path)
  bool xrev = false;
  bool use_graph = false;
  int cus = 0, lg_cap = 0, nblk = 0, msplit_n = 0;
  bool sampling = false, row_temps = false;
  // history rules (janus_decode_options.repetition_penalty / no_repeat_ngram_size): 1 and 0 = off
  float rep_pen = 1.f;
  int ngram = 0;
  // the cross-attention over the call's encoder rows quantised to int8 (janus_whisper_set_cross_compute)
  bool cross_i8 = false;
  // every decoder linear layer and the vocabulary projection on the int8 weights
  // (janus_whisper_set_decoder_compute): the unfused launch path
  bool dec_i8 = false;
  // ---- host arrays to upload
  std::vector<XPair> pairs;
  std::vector<int> groups;  // [ngroups][8] = {e, row_0 .. row_6 (-1: none)}
  int grp_rows = 0, rem_rows = 0, n_main = -1;   // (wide: groups [n_main, ngroups) hold <= rem_rows rows)
  std::vector<int32_t> plen;   // [B] prompt lengths
  std::vector<int32_t> init;   // [B][maxlen] initial token rows (prompt, then -1)
  std::vector<int32_t> roff;   // [B] staggered rows' offsets (empty: not staggered)
  std::vector<float> itemp;    // [B] per-row 1 / T (row_temps)
  DecodeRules R{};

  int npairs() const { return (int)pairs.size(); }
  int ngroups() const { return (int)groups.size() / 8; }
  bool stagger() const { return !roff.empty(); }
  bool shared() const { return enc_rows != JANUS_ENC_ROWS_OWN; }
  bool hist() const { return rep_pen != 1.f || ngram > 0; }

  // The scalar fields, once. step(name, value): what a captured position reads — the
  // graph cache key and operator== come from these. call(name, value): what only the code
  // around the positions reads (how many run, which rows are uploaded, what is reported):
  // calls that differ in these alone share their graphs.
  template <class F, class G> void each_scalar(F&& step, G&& call) const {
    step("B", B); step("maxlen", maxlen); step("chunk", chunk); step("sample_begin", sample_begin);
    step("max_roff", max_roff); step("nwin", nwin); step("beam_k", beam_k);
    step("wide", wide); step("xabs", xabs); step("xsplit", xsplit); step("cvp", cvp);
    step("fused_ln", fused_ln); step("ln_fuse", ln_fuse); step("ln_pro_mask", ln_pro_mask);
    step("embed_ln", embed_ln); step("rln", rln); step("fuse_se", fuse_se);
    step("seg_grid", seg_grid); step("persist", persist); step("xrev", xrev);
    step("lg_cap", lg_cap); step("nblk", nblk); step("msplit_n", msplit_n);
    step("sampling", sampling); step("row_temps", row_temps); step("stagger", stagger());
    step("npairs", npairs()); step("ngroups", ngroups()); step("grp_rows", grp_rows);
    step("rem_rows", rem_rows); step("n_main", n_main);
    step("R.eot", R.eot); step("R.suppress_blank", R.suppress_blank); step("R.blank", R.blank);
    step("R.ts_begin", R.ts_begin); step("R.no_timestamps", R.no_timestamps);
    step("R.max_initial_ts", R.max_initial_ts); step("R.target", R.target);
    step("R.inv_temp", R.inv_temp); step("no_speech_back", nsp_back);
    call("steps", steps); call("check_every", check_every); call("f0", f0); call("f1", f1);
    call("enc_rows", enc_rows); call("n_enc", n_enc); call("use_graph", use_graph); call("cus", cus);
  }
  // the plan's part of the graph cache key (LaneBuffers appends the device pointers)
  void append_key(std::vector<int64_t>& key) const {
    each_scalar([&](const char*, auto v) { key.push_back(key_word(v)); }, [](const char*, auto) {});
    // the history rules, only on a call that sets them: every other call's key is unchanged
    if (hist()) { key.push_back(key_word(rep_pen)); key.push_back(key_word(ngram)); }
    // likewise the int8 cross-attention: one tagged word, only when set
    if (cross_i8) key.push_back(kCrossI8KeyWord);
    if (dec_i8) key.push_back(kDecI8KeyWord);
  }
  bool operator==(const DecodePlan& o) const {
    std::vector<int64_t> a, b;
    append_key(a);
    o.append_key(b);
    return a == b;
  }
  // name=value lines (janus_decode_plan_describe): the step fields, the call fields as
  // call.name, then pairs= and groups= as integer lists; repetition_penalty= and
  // no_repeat_ngram_size= lines in front of pairs= only on a call that sets one of them, and
  // cross_int8=1 after them only on a call with the int8 cross-attention, dec_int8=1 after that
  // only on a call with the int8 decoder weights
  std::string describe() const;
};

// Checks the call's arguments (every rejection a janus::Error, before anything is enqueued)
// and decides its path. cus: the CUs of the caller's stream (stream_cu_count);
// multi_lane: the call is one lane of several running concurrently. cross_compute: the
// context's JANUS_CROSS_COMPUTE_* (janus_whisper_set_cross_compute); dec_compute: its
// JANUS_DEC_COMPUTE_* (janus_whisper_set_decoder_compute).
DecodePlan plan_decode(const janus_whisper_config& cfg, const janus_decode_options& opt,
                       const janus_decode_rows* rows, const DecodeSampling* smp, const BeamMode* beam,
                       int B, int cus, bool multi_lane, const LaneStand& stand, const SegDevice& seg,
                       int cross_compute = JANUS_CROSS_COMPUTE_F16, int dec_compute = JANUS_DEC_COMPUTE_F16);

}  // namespace janus

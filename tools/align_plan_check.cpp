// Stand-alone driver of the host-only alignment plan (janus_amd/csrc/align_plan.cpp): layout
// and every rejection of janus_whisper_align's validation, without HIP or a device. Build and
// run, plain or under the host sanitizers (tests/test_align_host.py runs the plain build):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I janus_amd/csrc tools/align_plan_check.cpp \
//       janus_amd/csrc/align_plan.cpp -o /tmp/align_plan_check && /tmp/align_plan_check
#include <algorithm>
#include <cstdio>
#include <vector>
#include "align_plan.h"
using namespace janus;
static int expect_throw(const char* what, void (*f)()) {
  try { f(); } catch (const Error& e) { std::printf("ok  %-28s %s\n", what, e.what()); return 0; }
  std::printf("FAIL %s did not throw\n", what); return 1;
}
static std::vector<int32_t> seq(int text, int eot = 50256) {
  std::vector<int32_t> s{50257, 50362};
  for (int i = 0; i < text; ++i) s.push_back(300 + i);
  s.push_back(eot);
  return s;
}
static AlignPlan plan(const std::vector<std::vector<int32_t>>& seqs, const std::vector<int32_t>& sizes,
                      const std::vector<int32_t>* ei, int n_enc, int ps = 2000) {
  int stride = 1;
  for (auto& s : seqs) stride = std::max<int>(stride, s.size());
  std::vector<int32_t> toks(seqs.size() * stride, 0), lens;
  for (size_t w = 0; w < seqs.size(); ++w) {
    std::copy(seqs[w].begin(), seqs[w].end(), toks.begin() + w * stride);
    lens.push_back((int32_t)seqs[w].size());
  }
  return align_plan(448, 51864, 12, n_enc, (int)seqs.size(), toks.data(), lens.data(), stride, sizes.data(),
                    ei ? ei->data() : nullptr, 1, 50256, ps);
}
int main() {
  int bad = 0;
  std::vector<int32_t> ei{1, 0, 1};
  AlignPlan P = plan({seq(1), seq(33), seq(445)}, {3000, 437, 6}, &ei, 2);
  std::printf("M %d tiles %d probs %lld A %lld trace %lld\n", P.M, P.n_tiles(), (long long)P.probs_total,
              (long long)P.a_total, (long long)P.trace_total);
  bad += !(P.M == 4 + 36 + 448 && P.n_tiles() == 1 + 3 + 28 && P.wins[2].F == 3 && P.wins[2].N == 446);
  bad += !(P.target[1] == 300 && P.target[0] == -1 && P.target[2] == -1 && P.out_idx[1] == 0);
  bad += !(P.out_idx[4 + 1] == 448 && P.target[4 + 33] == 332 && P.target[4 + 34] == -1);
  bad += expect_throw("no text", [] { plan({seq(0)}, {3000}, nullptr, 1); });
  bad += expect_throw("too long", [] { plan({seq(446)}, {3000}, nullptr, 1); });
  bad += expect_throw("size 1", [] { plan({seq(3)}, {1}, nullptr, 1); });
  bad += expect_throw("size 3001", [] { plan({seq(3)}, {3001}, nullptr, 1); });
  bad += expect_throw("enc rows", [] { plan({seq(3), seq(3)}, {3000, 3000}, nullptr, 1); });
  bad += expect_throw("enc_index", [] { std::vector<int32_t> e{2}; plan({seq(3)}, {3000}, &e, 2); });
  bad += expect_throw("no eot", [] { plan({seq(3, 7)}, {3000}, nullptr, 1); });
  bad += expect_throw("path stride", [] { plan({seq(3)}, {3000}, nullptr, 1, 100); });
  bad += expect_throw("text >= eot", [] { auto s = seq(3); s[3] = 50300; plan({s}, {3000}, nullptr, 1); });
  std::vector<int32_t> h = align_default_heads(4, 6);
  bad += !(h.size() == 24 && h[0] == 2 && h[23] == 5);
  align_check_heads(4, 6, h.data(), 12);
  bad += expect_throw("heads range", [] { int32_t p[2] = {4, 0}; align_check_heads(4, 6, p, 1); });
  bad += expect_throw("heads twice", [] { int32_t p[4] = {1, 0, 1, 0}; align_check_heads(4, 6, p, 2); });
  bad += expect_throw("heads none", [] { align_check_heads(4, 6, nullptr, 0); });
  bad += expect_throw("default > 64", [] { align_default_heads(32, 20); });
  std::printf(bad ? "FAILED\n" : "all ok\n");
  return bad;
}

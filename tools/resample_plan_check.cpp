// Stand-alone driver of the host-only resampler plan (janus_amd/csrc/resample_plan.cpp): walks
// resample_kernel's index arithmetic (csrc/resample.hip) on the host over the staging layout
// janus_resample_f32 uses, with every staging, table and output access bounds-checked
// (std::vector::at), and compares each output with the plan's taps applied directly in double.
// No HIP, no device. Build and run, plain or under the host sanitizers
// (tests/test_resample_host.py runs the plain build):
//   g++ -std=c++17 -g -fsanitize=address,undefined -I janus_amd/csrc tools/resample_plan_check.cpp \
//       janus_amd/csrc/resample_plan.cpp -o /tmp/resample_plan_check && /tmp/resample_plan_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "errors.h"
#include "resample_plan.h"
using namespace janus;

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

static int run(int sr_in, int sr_out, const std::vector<int64_t>& lens) {
  const ResamplePlan P = make_resample_plan(sr_in, sr_out);
  const ResampleTiles R = make_resample_tiles(P);
  const int n_clips = (int)lens.size();
  std::vector<int64_t> offs(n_clips + 1, 0), obase(n_clips + 1, 0);
  int64_t max_out = 0;
  for (int c = 0; c < n_clips; ++c) {
    offs[c + 1] = offs[c] + lens[c];
    obase[c + 1] = obase[c] + resample_out_len(P, lens[c]);
    max_out = std::max(max_out, resample_out_len(P, lens[c]));
  }
  const ResampleStage S = resample_stage_layout(P, R, offs.data(), n_clips);
  std::vector<float> x(offs[n_clips]), stage(S.total, 0.0f), out(obase[n_clips], -777.0f);
  uint32_t seed = 12345u;
  for (auto& v : x) {
    seed = seed * 1664525u + 1013904223u;
    v = (float)(seed >> 8) / 16777216.0f - 0.5f;
  }
  for (int c = 0; c < n_clips; ++c)   // resample_stage_kernel
    for (int64_t i = 0; i < lens[c]; ++i) stage.at(S.base[c] + i) = x[offs[c] + i];
  int64_t written = 0;
  const int64_t blocks = cdiv(cdiv(max_out, R.Lg), kResampleBlockRows);
  for (int c = 0; c < n_clips; ++c)   // resample_kernel: block (bx, c), wave w, lane (l15 = row | column, l4)
    for (int64_t bx = 0; bx < blocks; ++bx)
      for (int w = 0; w < kResampleWaves; ++w) {
        const int64_t n_out = obase[c + 1] - obase[c], rows = cdiv(n_out, R.Lg);
        const int64_t row0 = (bx * kResampleWaves + w) * (16 * kResampleRowTiles);
        if (row0 >= rows) continue;
        for (int j = 0; j < R.n_ct; ++j) {
          const int kstart = R.meta[3 * j], ksteps = R.meta[3 * j + 1], ofs = R.meta[3 * j + 2];
          for (int m = 0; m < kResampleRowTiles; ++m) {
            const bool ok = row0 + 16 * m < rows;
            for (int row = 0; row < 16; ++row)
              for (int col = 0; col < 16; ++col) {
                float acc = 0.0f;
                for (int kk = 0; kk < ksteps; ++kk)
                  for (int l4 = 0; l4 < 4; ++l4) {
                    const float a = stage.at(S.base[c] + (row0 + (ok ? 16 * m : 0) + row) * R.Mg + l4 + kstart + 4 * kk);
                    const float b = R.table.at((size_t)ofs + (size_t)kk * 64 + l4 * 16 + col);
                    acc = std::fmaf(a, b, acc);
                  }
                const int64_t idx = (row0 + 16 * m + row) * R.Lg + 16 * j + col;
                if (16 * j + col < R.Lg && ok && idx < n_out) {
                  out.at(obase[c] + idx) = acc;
                  ++written;
                }
              }
          }
        }
      }
  if (written != obase[n_clips]) {
    std::printf("FAIL %d -> %d: %lld of %lld outputs written\n", sr_in, sr_out, (long long)written,
                (long long)obase[n_clips]);
    return 1;
  }
  double worst = 0.0;
  for (int c = 0; c < n_clips; ++c)
    for (int64_t n = 0; n < obase[c + 1] - obase[c]; ++n) {
      const int p = (int)(n % P.L);
      const int64_t i = n / P.L;
      double y = 0.0;
      for (int t = 0; t < P.count[p]; ++t) {
        const int64_t xi = i * P.M + P.first[p] + t;
        if (xi >= 0 && xi < lens[c]) y += (double)P.taps[(size_t)p * P.T + t] * x[offs[c] + xi];
      }
      worst = std::max(worst, std::fabs(y - out[obase[c] + n]));
    }
  // (T + 4) 2^-24 ||h||_1 max|x| with ||h||_1 <= 2.77, max|x| <= 0.5
  const double bound = (P.T + 4) * std::ldexp(1.0, -24) * 2.77 * 0.5;
  std::printf("%s %6d -> %6d: L %3d M %3d T %3d G %2d tiles %2d k [%d, %d) front %lld stage %lld worst %.3g\n",
              worst <= bound ? "ok  " : "FAIL", sr_in, sr_out, P.L, P.M, P.T, R.G, R.n_ct, R.kmin, R.kend,
              (long long)S.front, (long long)S.total, worst);
  return worst <= bound ? 0 : 1;
}

static int expect_throw(int sr_in, int sr_out) {
  try {
    make_resample_plan(sr_in, sr_out);
  } catch (const Error& e) {
    std::printf("ok   refused: %s\n", e.what());
    return 0;
  }
  std::printf("FAIL %d -> %d did not throw\n", sr_in, sr_out);
  return 1;
}

int main() {
  int bad = 0;
  const int pairs[][2] = {{44100, 16000}, {48000, 16000}, {8000, 16000},   {11025, 16000},  {44100, 48000},
                          {16000, 48000}, {22050, 16000}, {192000, 16000}, {176400, 16000}, {12000, 16000}};
  for (const auto& pr : pairs) {
    const ResamplePlan P = make_resample_plan(pr[0], pr[1]);
    const int64_t tile_in = (int64_t)kResampleBlockRows * make_resample_tiles(P).Lg * P.M / P.L;
    bad += run(pr[0], pr[1], {1, 0, 2, P.M - 1, P.M, P.M + 1, 16 * P.M - 1, 16 * P.M + 1, tile_in - 1, tile_in,
                              tile_in + 1, tile_in + P.M, 5000});
  }
  bad += expect_throw(44101, 16000) + expect_throw(3999, 16000) + expect_throw(0, 16000) + expect_throw(16000, 384001);
  std::printf(bad ? "FAILED\n" : "all ok\n");
  return bad ? 1 : 0;
}

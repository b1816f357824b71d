// Host plan of the band-limited resampler: see resample_plan.h and the rule in
// include/janus.h. Every index is integer arithmetic on r = p M mod L and Wn = Z max(L, M)
// (u = (r - k L) / L, W = Wn / L), so which taps a phase has never hangs on a rounding.
#include "resample_plan.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>
#include <string>
#include "errors.h"

namespace janus {

// I0 by its power series sum_k ((x / 2)^2k / (k!)^2): all terms positive, so it converges to
// double precision without cancellation (x <= beta = 10: 40 terms).
static double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

ResamplePlan make_resample_plan(int sr_in, int sr_out) {
  const std::string name = "resample " + std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " Hz";
  JANUS_CHECK(sr_in >= kResampleMinRate && sr_in <= kResampleMaxRate && sr_out >= kResampleMinRate &&
                  sr_out <= kResampleMaxRate,
              name + ": both rates must lie in " + std::to_string(kResampleMinRate) + " .. " +
                  std::to_string(kResampleMaxRate));
  ResamplePlan P;
  P.sr_in = sr_in;
  P.sr_out = sr_out;
  const int g = std::gcd(sr_in, sr_out);
  P.L = sr_out / g;
  P.M = sr_in / g;
  JANUS_CHECK(P.L <= kResampleMaxPhases, name + ": the pair reduces to " + std::to_string(P.L) + " / " +
                                             std::to_string(P.M) + ", more than " +
                                             std::to_string(kResampleMaxPhases) + " phases");
  const int64_t L = P.L, M = P.M;
  if (L == 1 && M == 1) {
    P.copy = true;
    P.T = 1;
    P.first = {0};
    P.count = {1};
    P.taps = {1.0f};
    return P;
  }
  const int64_t D = std::max(L, M), Wn = (int64_t)kResampleZeros * D;
  const double s = (double)L / (double)D;   // min(1, L / M)
  P.half_width = (int)ceil_div(Wn, L);
  P.first.resize(L);
  P.count.resize(L);
  std::vector<int64_t> kmin(L);
  int T = 0;
  for (int64_t p = 0; p < L; ++p) {
    const int64_t r = (p * M) % L, c = (p * M) / L;
    // |r - k L| < Wn: k in (floor((r - Wn) / L), ceil((r + Wn) / L))
    kmin[p] = floor_div(r - Wn, L) + 1;
    const int64_t kmax = ceil_div(r + Wn, L) - 1;
    P.first[p] = (int32_t)(c + kmin[p]);
    P.count[p] = (int32_t)(kmax - kmin[p] + 1);
    T = std::max(T, P.count[p]);
  }
  P.T = T;
  P.taps.assign((size_t)L * T, 0.0f);
  const double inv_i0 = 1.0 / bessel_i0(kResampleBeta);
  const double pi = 3.14159265358979323846;
  std::vector<double> h(T);
  for (int64_t p = 0; p < L; ++p) {
    const int64_t r = (p * M) % L;
    double sum = 0.0;
    for (int t = 0; t < P.count[p]; ++t) {
      const int64_t d = r - (kmin[p] + t) * L;              // u = d / L
      const double uw = (double)d / (double)Wn;             // u / W
      const double v = (double)d / (double)D;               // s u
      const double sinc = d == 0 ? 1.0 : std::sin(pi * v) / (pi * v);
      const double win = bessel_i0(kResampleBeta * std::sqrt(std::max(0.0, 1.0 - uw * uw))) * inv_i0;
      h[t] = s * sinc * win;
      sum += h[t];
    }
    for (int t = 0; t < P.count[p]; ++t) P.taps[(size_t)p * T + t] = (float)(h[t] / sum);  // the one rounding
  }
  return P;
}

ResampleTiles make_resample_tiles(const ResamplePlan& P) {
  ResampleTiles R;
  R.G = P.L >= 16 ? 1 : 16 / std::gcd(P.L, 16);
  R.Lg = R.G * P.L;
  R.Mg = R.G * P.M;
  R.n_ct = (R.Lg + 15) / 16;
  R.meta.resize((size_t)R.n_ct * 3);
  R.kmin = INT_MAX;
  R.kend = INT_MIN;
  for (int j = 0; j < R.n_ct; ++j) {
    int lo = INT_MAX, hi = INT_MIN;
    for (int n = 16 * j; n < std::min(16 * j + 16, R.Lg); ++n) {
      const int start = (n / P.L) * P.M + P.first[n % P.L];
      lo = std::min(lo, start);
      hi = std::max(hi, start + P.count[n % P.L]);
    }
    const int ksteps = (hi - lo + 3) / 4, ofs = (int)R.table.size();
    R.meta[3 * j] = lo;
    R.meta[3 * j + 1] = ksteps;
    R.meta[3 * j + 2] = ofs;
    R.table.resize((size_t)ofs + (size_t)ksteps * 64, 0.0f);
    for (int n = 16 * j; n < std::min(16 * j + 16, R.Lg); ++n) {
      const int p = n % P.L, start = (n / P.L) * P.M + P.first[p];
      for (int t = 0; t < P.count[p]; ++t) {
        const int k = start + t - lo;
        R.table[(size_t)ofs + (size_t)(k >> 2) * 64 + (k & 3) * 16 + (n - 16 * j)] = P.taps[(size_t)p * P.T + t];
      }
    }
    R.kmin = std::min(R.kmin, lo);
    R.kend = std::max(R.kend, lo + 4 * ksteps);
  }
  return R;
}

int64_t resample_front_zeros(const ResamplePlan& P) { return ((int64_t)P.half_width + 1 + 15) / 16 * 16; }

ResampleStage resample_stage_layout(const ResamplePlan& P, const ResampleTiles& R, const int64_t* offsets,
                                    int n_clips) {
  ResampleStage S;
  S.front = resample_front_zeros(P);
  JANUS_CHECK(-R.kmin <= S.front, "resample plan: taps reach past the front zeros");
  S.base.resize(n_clips);
  for (int c = 0; c < n_clips; ++c) {
    const int64_t n = offsets[c + 1] - offsets[c], n_out = resample_out_len(P, n);
    const int64_t rows16 = ((n_out + R.Lg - 1) / R.Lg + 15) / 16 * 16;
    const int64_t behind = rows16 > 0 ? std::max(n, (rows16 - 1) * R.Mg + R.kend) : 0;
    S.base[c] = S.total + S.front;
    S.total += S.front + (behind + 15) / 16 * 16;
  }
  return S;
}

}  // namespace janus

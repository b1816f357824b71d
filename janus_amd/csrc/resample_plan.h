// The plan of one rate pair of the band-limited resampler (include/janus.h states the rule):
// the reduced pair, the polyphase tap table in float64 rounded once to float32, and the same
// taps laid out as the banded matrix of resample.hip's GEMM. Host only: no device work, no
// HIP header, like decode_plan.
#pragma once
#include <cstdint>
#include <vector>

namespace janus {

constexpr int kResampleZeros = 32;         // Z: zero crossings on each side at the cutoff
constexpr double kResampleBeta = 10.0;     // Kaiser beta
constexpr int kResampleMaxPhases = 640;    // the reduced L may not exceed it
constexpr int kResampleMinRate = 4000, kResampleMaxRate = 384000;

struct ResamplePlan {
  int sr_in = 0, sr_out = 0;
  int L = 1, M = 1;            // sr_out / gcd, sr_in / gcd
  int T = 1;                   // taps of the widest phase: the row length of `taps`
  int half_width = 0;          // ceil(W), W = Z / min(1, L / M) in input samples
  bool copy = false;           // sr_in == sr_out: one tap of 1
  std::vector<int32_t> first;  // [L] c_p + kmin_p: output i L + p starts at x[i M + first[p]]
  std::vector<int32_t> count;  // [L] taps of phase p (<= T; the row is zero beyond)
  std::vector<float> taps;     // [L][T]
};

// Throws janus::Error naming both rates for a rate outside 4000 .. 384000 or a reduced L
// above 640.
ResamplePlan make_resample_plan(int sr_in, int sr_out);

inline int64_t resample_out_len(const ResamplePlan& p, int64_t n_in) {
  return (n_in * p.L + p.M - 1) / p.M;
}

// resample_kernel's block: 4 waves, each 2 row tiles of 16 rows
constexpr int kResampleWaves = 4, kResampleRowTiles = 2;
constexpr int kResampleBlockRows = 16 * kResampleRowTiles * kResampleWaves;  // rows of Lg outputs per block

// The GEMM view. G periods form one row (G = 1 for L >= 16, else 16 / gcd(L, 16), so that a
// row holds a whole number of 16-column tiles): row r, column n of Lg = G L outputs is
// output r Lg + n, drawn from x[r Mg + kstart[j] ...), Mg = G M, j = n / 16. Column tile j
// reads 4 ksteps[j] inputs per row; its taps stand in `table` from tabofs[j] on as
// [kstep][k & 3][column] (the MFMA's B fragment: one coalesced load per step), zero where a
// column has no tap.
struct ResampleTiles {
  int G = 1, Lg = 1, Mg = 1, n_ct = 0;
  int kmin = 0, kend = 0;            // every row reads x[r Mg + kmin .. r Mg + kend)
  std::vector<int32_t> meta;         // [n_ct][3]: kstart, ksteps, tabofs
  std::vector<float> table;
};
ResampleTiles make_resample_tiles(const ResamplePlan& p);

// The staging buffer of one call: clip c sits at [base[c], base[c] + n_in[c]) with `front`
// zeros before it (ceil(W) + 1, rounded up to 16 floats) and zeros behind it up to the last
// read of its last 16-row tile, (rows16 - 1) Mg + kend; `total` floats in all. Every A read
// of resample_kernel for clip c then lies in [base[c] - front, the next clip's span).
struct ResampleStage {
  int64_t front = 0, total = 0;
  std::vector<int64_t> base;
};
int64_t resample_front_zeros(const ResamplePlan& p);
ResampleStage resample_stage_layout(const ResamplePlan& p, const ResampleTiles& t, const int64_t* offsets,
                                    int n_clips);

}  // namespace janus

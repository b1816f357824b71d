// C-ABI of the band-limited resampler (resample.hip): a resampler object holds the plan of
// one rate pair, its tap matrix on the device and the grow-only staging buffer that gives
// every clip the zeros the rule extends it with.
#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>
#include "devmem.h"
#include "kernels.h"
#include "resample_plan.h"
#include "../../include/janus.h"

struct janus_resampler {
  janus::ResamplePlan plan;
  janus::ResampleTiles tiles;
  janus::DevMem table, tile_meta, stage, meta;   // stage, meta: grow-only
  std::vector<int64_t> meta_host;
  std::mutex mu;
};

using namespace janus;

extern "C" int janus_resample_plan(int sr_in, int sr_out, int* L, int* M, int* T, int32_t* first,
                                   int64_t first_capacity, float* taps, int64_t taps_capacity) {
  return guarded([&] {
    const ResamplePlan P = make_resample_plan(sr_in, sr_out);
    if (L) *L = P.L;
    if (M) *M = P.M;
    if (T) *T = P.T;
    if (first) {
      JANUS_CHECK(first_capacity >= P.L, "resample plan: first needs " + std::to_string(P.L) + " entries");
      std::copy(P.first.begin(), P.first.end(), first);
    }
    if (taps) {
      JANUS_CHECK(taps_capacity >= (int64_t)P.taps.size(),
                  "resample plan: taps needs " + std::to_string(P.taps.size()) + " entries");
      std::copy(P.taps.begin(), P.taps.end(), taps);
    }
  });
}

extern "C" int janus_resampler_create(int sr_in, int sr_out, janus_resampler** out) {
  return guarded([&] {
    JANUS_CHECK(out, "null argument");
    *out = nullptr;
    ResamplePlan P = make_resample_plan(sr_in, sr_out);
    auto r = std::make_unique<janus_resampler>();
    r->plan = std::move(P);
    if (!r->plan.copy) {
      r->tiles = make_resample_tiles(r->plan);
      const ResampleTiles& R = r->tiles;
      JANUS_CHECK(-R.kmin <= resample_front_zeros(r->plan), "resample plan: taps reach past the front zeros");
      r->table.ensure(sizeof(float) * R.table.size());
      r->tile_meta.ensure(sizeof(int32_t) * R.meta.size());
      JANUS_HIP(hipMemcpy(r->table.p, R.table.data(), sizeof(float) * R.table.size(), hipMemcpyHostToDevice));
      JANUS_HIP(hipMemcpy(r->tile_meta.p, R.meta.data(), sizeof(int32_t) * R.meta.size(), hipMemcpyHostToDevice));
    }
    *out = r.release();
  });
}

extern "C" int janus_resampler_destroy(janus_resampler* r) {
  return guarded([&] {
    if (r) {
      (void)hipDeviceSynchronize();
      delete r;
    }
  });
}

extern "C" int janus_resampler_info(const janus_resampler* r, int* L, int* M, int* T, int* out_tile,
                                    int* front) {
  return guarded([&] {
    JANUS_CHECK(r, "null argument");
    if (L) *L = r->plan.L;
    if (M) *M = r->plan.M;
    if (T) *T = r->plan.T;
    if (out_tile) *out_tile = r->plan.copy ? 1 : kResampleBlockRows * r->tiles.Lg;
    if (front) *front = r->plan.copy ? 0 : (int)resample_front_zeros(r->plan);
  });
}

extern "C" int janus_resample_f32(janus_resampler* r, const float* pcm, const int64_t* offsets,
                                  int n_clips, float* out, const int64_t* out_offsets, void* stream) {
  return guarded([&] {
    JANUS_CHECK(r && n_clips >= 0, "bad argument");
    if (n_clips == 0) return;
    JANUS_CHECK(offsets && out_offsets, "null argument");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(r->mu);
    const ResamplePlan& P = r->plan;
    int64_t max_in = 0, max_out = 0;
    for (int c = 0; c < n_clips; ++c) {
      const int64_t n = offsets[c + 1] - offsets[c];
      JANUS_CHECK(n >= 0, "resample: offsets must not decrease");
      JANUS_CHECK(out_offsets[c + 1] - out_offsets[c] == resample_out_len(P, n),
                  "resample: out_offsets must give clip " + std::to_string(c) + " ceil(n_in L / M) = " +
                      std::to_string(resample_out_len(P, n)) + " samples");
      max_in = std::max(max_in, n);
      max_out = std::max(max_out, resample_out_len(P, n));
    }
    if (max_in == 0) return;   // nothing to read, nothing to write
    JANUS_CHECK(pcm && out, "null argument");
    if (P.copy) {
      for (int c = 0; c < n_clips; ++c)
        if (offsets[c + 1] > offsets[c])
          JANUS_HIP(hipMemcpyAsync(out + out_offsets[c], pcm + offsets[c],
                                   sizeof(float) * (offsets[c + 1] - offsets[c]), hipMemcpyDeviceToDevice, s));
      return;
    }
    const ResampleTiles& R = r->tiles;
    // per clip: [front zeros | samples | zeros to the end of its last 16-row tile's reads]
    const ResampleStage S = resample_stage_layout(P, R, offsets, n_clips);
    const int64_t total = S.total;
    std::vector<int64_t>& mh = r->meta_host;
    mh.assign(5 * (size_t)n_clips, 0);
    for (int c = 0; c < n_clips; ++c) {
      const int64_t n = offsets[c + 1] - offsets[c];
      mh[c] = offsets[c];
      mh[n_clips + c] = n;
      mh[2 * (size_t)n_clips + c] = S.base[c];
      mh[3 * (size_t)n_clips + c] = out_offsets[c];
      mh[4 * (size_t)n_clips + c] = resample_out_len(P, n);
    }
    r->meta.ensure(sizeof(int64_t) * mh.size());
    r->stage.ensure(sizeof(float) * (size_t)total);
    // pageable source: staged before the call returns; meta_host lives in the object
    JANUS_HIP(hipMemcpyAsync(r->meta.p, mh.data(), sizeof(int64_t) * mh.size(), hipMemcpyHostToDevice, s));
    JANUS_HIP(hipMemsetAsync(r->stage.p, 0, sizeof(float) * (size_t)total, s));
    resample_launch(pcm, r->meta.as<int64_t>(), n_clips, max_in, max_out, r->stage.as<float>(),
                    r->tile_meta.as<int32_t>(), r->table.as<float>(), R.Lg, R.Mg, R.n_ct, out, s);
  });
}

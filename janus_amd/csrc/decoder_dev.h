// Device-side helpers shared by the selectors of decoder.hip and the beam kernels of
// beam.hip: the same code on both sides, so a beam of one row reduces a row's partials in
// the same order as the greedy selector (bit-identical statistics).
#pragma once
#include "mfma.h"
#include "decoder.h"

namespace janus {

__device__ __forceinline__ float lse_merge(float m1, float s1, float m2, float s2, float* mo) {
  const float m = fmaxf(m1, m2);
  *mo = m;
  if (m == -INFINITY) return 0.f;
  return s1 * __expf(m1 - m) + s2 * __expf(m2 - m);
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// 256 threads: the nblk partials of one row (pr) merged into one LogitPart, returned in
// thread 0 (the other threads' return value is meaningless). sh: 4 LogitParts of LDS. Ends
// with a __syncthreads() behind every wave's write to sh, none after thread 0's reads: a
// caller that reuses sh synchronises first.
__device__ __forceinline__ LogitPart row_parts_reduce(const LogitPart* __restrict__ pr, int nblk,
                                                      LogitPart* sh) {
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  float m_all = -INFINITY, s_all = 0.f, m_text = -INFINITY, m_ts = -INFINITY, s_ts = 0.f;
  float ba_v = -INFINITY, bt_v = -INFINITY;
  int ba_i = 0x7fffffff, bt_i = 0x7fffffff;
  float m_raw = -INFINITY, s_raw = 0.f, t_v = -INFINITY;
  float ba_r = -INFINITY, bt_r = -INFINITY;
  for (int i = tid; i < nblk; i += 256) {
    const LogitPart p = pr[i];
    float mo;
    s_all = lse_merge(m_all, s_all, p.m_all, p.s_all, &mo); m_all = mo;
    s_ts = lse_merge(m_ts, s_ts, p.m_ts, p.s_ts, &mo); m_ts = mo;
    s_raw = lse_merge(m_raw, s_raw, p.m_raw, p.s_raw, &mo); m_raw = mo;
    m_text = fmaxf(m_text, p.m_text);
    t_v = fmaxf(t_v, p.t_v);
    if (better(p.b_all_v, p.b_all_i, ba_v, ba_i)) { ba_v = p.b_all_v; ba_i = p.b_all_i; ba_r = p.b_all_r; }
    if (better(p.b_ts_v, p.b_ts_i, bt_v, bt_i)) { bt_v = p.b_ts_v; bt_i = p.b_ts_i; bt_r = p.b_ts_r; }
  }
  // butterfly over the wave (xshfl: the partner lane's values as __shfl_xor, no LDS trip)
  auto level = [&](auto shf, auto shi) __attribute__((always_inline)) {
    float mo;
    const float om = shf(m_all), os = shf(s_all);
    s_all = lse_merge(m_all, s_all, om, os, &mo); m_all = mo;
    const float tm = shf(m_ts), ts = shf(s_ts);
    s_ts = lse_merge(m_ts, s_ts, tm, ts, &mo); m_ts = mo;
    const float rm = shf(m_raw), rs = shf(s_raw);
    s_raw = lse_merge(m_raw, s_raw, rm, rs, &mo); m_raw = mo;
    m_text = fmaxf(m_text, shf(m_text));
    t_v = fmaxf(t_v, shf(t_v));
    const float av = shf(ba_v); const int ai = shi(ba_i);
    const float ar = shf(ba_r);
    if (better(av, ai, ba_v, ba_i)) { ba_v = av; ba_i = ai; ba_r = ar; }
    const float tv = shf(bt_v); const int ti = shi(bt_i);
    const float tr = shf(bt_r);
    if (better(tv, ti, bt_v, bt_i)) { bt_v = tv; bt_i = ti; bt_r = tr; }
  };
  level([](float x) { return xshfl<32>(x); }, [](int x) { return xshfl_i<32>(x); });
  level([](float x) { return xshfl<16>(x); }, [](int x) { return xshfl_i<16>(x); });
  level([](float x) { return xshfl<8>(x); }, [](int x) { return xshfl_i<8>(x); });
  level([](float x) { return xshfl<4>(x); }, [](int x) { return xshfl_i<4>(x); });
  level([](float x) { return xshfl<2>(x); }, [](int x) { return xshfl_i<2>(x); });
  level([](float x) { return xshfl<1>(x); }, [](int x) { return xshfl_i<1>(x); });
  LogitPart q;
  q.m_all = m_all; q.s_all = s_all; q.m_text = m_text; q.m_ts = m_ts; q.s_ts = s_ts;
  q.b_all_v = ba_v; q.b_all_i = ba_i; q.b_ts_v = bt_v; q.b_ts_i = bt_i;
  q.t_v = t_v; q.m_raw = m_raw; q.s_raw = s_raw; q.b_all_r = ba_r; q.b_ts_r = bt_r;
  if (lane == 0) sh[w] = q;
  __syncthreads();
  if (tid != 0) return q;
  for (int k = 1; k < 4; ++k) {
    const LogitPart& p = sh[k];
    float mo;
    s_all = lse_merge(m_all, s_all, p.m_all, p.s_all, &mo); m_all = mo;
    s_ts = lse_merge(m_ts, s_ts, p.m_ts, p.s_ts, &mo); m_ts = mo;
    s_raw = lse_merge(m_raw, s_raw, p.m_raw, p.s_raw, &mo); m_raw = mo;
    m_text = fmaxf(m_text, p.m_text);
    t_v = fmaxf(t_v, p.t_v);
    if (better(p.b_all_v, p.b_all_i, ba_v, ba_i)) { ba_v = p.b_all_v; ba_i = p.b_all_i; ba_r = p.b_all_r; }
    if (better(p.b_ts_v, p.b_ts_i, bt_v, bt_i)) { bt_v = p.b_ts_v; bt_i = p.b_ts_i; bt_r = p.b_ts_r; }
  }
  q.m_all = m_all; q.s_all = s_all; q.m_text = m_text; q.m_ts = m_ts; q.s_ts = s_ts;
  q.b_all_v = ba_v; q.b_all_i = ba_i; q.b_ts_v = bt_v; q.b_ts_i = bt_i;
  q.t_v = t_v; q.m_raw = m_raw; q.s_raw = s_raw; q.b_all_r = ba_r; q.b_ts_r = bt_r;
  return q;
}

// The next step's rule state of a row whose state was r, whose last token (at the position
// the logits came from) was prev_tok and which now takes `next`.
__device__ __forceinline__ RowRules next_row_rules(RowRules r, const DecodeRules& R, int prev_tok,
                                                   int next) {
  const bool last_ts = R.ts_begin >= 0 && next >= R.ts_begin;
  const bool pen_ts = r.sample_begin || (R.ts_begin >= 0 && prev_tok >= R.ts_begin);
  r.sample_begin = 0;
  r.suppress_all_ts = last_ts && pen_ts;
  r.suppress_text = last_ts && !pen_ts;
  if (last_ts) r.last_stamp = next;
  r.ts_floor = r.last_stamp >= 0 ? ((last_ts && !pen_ts) ? r.last_stamp : r.last_stamp + 1) : -1;
  return r;
}

}  // namespace janus

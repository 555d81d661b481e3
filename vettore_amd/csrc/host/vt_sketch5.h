// vt_sketch5.h -- the host side of the 5-bit sketch (K1f: vt_sketch_nibble.hip the builders and the pass): the sums
// that bound the query level kept off its one-bit L plane, and a restatement of the row quantiser.  The query's
// signed-nibble levels are the 6-bit sketch's (vt_sketch6.h, sketch6_query_levels), used as they are.  Stand-alone on
// purpose (no HIP, no header of the library but vt_sketch6.h): vt_sketchsearch.h uses it, and tests/sketch5_check.cpp builds it
// with plain g++ under AddressSanitizer and UBSan.
#pragma once

#include "vt_sketch6.h"

namespace vt_host {

// 1-KiB runs of a 64-row tile: ld8 / 32 of H, ld8 / 128 of L, one of metadata
constexpr uint32_t sketch5_runs(uint32_t d) { return 5 * (sketch6_ld8(d) / 128) + 1; }

// What the pass needs to bound the level it keeps off the L plane.  Here 0 <= L_i <= 1, so Q.L lies in [*neg, *pos] (the
// sums of the level's negative and positive entries, sketch6_level_sums): the pass adds *c = 0.5 t (*pos + *neg) to the
// sum s_r multiplies and s_r *w with *w = 0.5 t ||Q||_1 to e_r.  Both products are exact in f64 (24 bits times 20).
inline void sketch5_level_bound(const uint32_t *level, uint32_t lw, float t, double *c, double *w) {
  int64_t pos = 0, neg = 0, l1 = 0;
  sketch6_level_sums(level, lw, &pos, &neg, &l1);
  const double half = 0.5 * (double)t;
  *c = half * (double)(pos + neg);
  *w = half * (double)l1;
}

// The row quantiser as nibble_row (vt_sketch_nibble.cuh) has it: s = max|x| / 15 in f32, X = round(x * (15 / max|x|)) clamped
// to [-15, 15]; X = 2 H + L with H = X >> 1 in [-8, 7] and L = X & 1.  rho >= ||x - s X|| and nu >= s ||X||, from f64
// sums with a 2^-30 margin, rounded up to f32.  (The device sums in another order: its bounds may differ in the last bits.)
inline void sketch5_quantise_row(const float *x, uint32_t d, int8_t *X, float *s_out, float *rho_out, float *nu_out) {
  float m = 0.0f;
  for (uint32_t i = 0; i < d; ++i) m = std::max(m, std::fabs(x[i]));
  float s = m / 15.0f;
  const float inv = 15.0f / m;
  const bool quantise = m > 0.0f && std::isfinite(inv) && s > 0.0f;
  if (!quantise) s = 0.0f;
  double res = 0.0, xx = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    int v = 0;
    if (quantise) {
      v = (int)std::nearbyint(x[i] * inv);
      v = v > 15 ? 15 : (v < -15 ? -15 : v);
    }
    X[i] = (int8_t)v;
    const double r = (double)x[i] - (double)s * (double)v;
    res += r * r;
    xx += (double)(v * v);
  }
  auto up = [](double v) {
    const float f = (float)v;
    return (double)f < v ? std::nextafterf(f, INFINITY) : f;
  };
  *s_out = s;
  *rho_out = up(std::sqrt(res) * (1.0 + 0x1p-30));
  *nu_out = up((double)s * std::sqrt(xx) * (1.0 + 0x1p-30));
}

// The two planes of a quantised row: H[i] = X[i] >> 1 (arithmetic), L[i] = X[i] & 1; X[i] = 2 H[i] + L[i].
inline void sketch5_split(const int8_t *X, uint32_t d, int8_t *H, uint8_t *L) {
  for (uint32_t i = 0; i < d; ++i) {
    const int v = X[i];
    L[i] = (uint8_t)(v & 1);
    H[i] = (int8_t)((v - (v & 1)) / 2);
  }
}

}  // namespace vt_host

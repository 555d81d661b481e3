// vt_sketch6.h -- the host side of the 6-bit sketch (K1s: vt_sketch_nibble.hip the builders and the pass):
// the query's signed-nibble levels, the sums that bound the level kept off the L plane and the bound itself, and a
// restatement of the row quantiser.  Stand-alone on purpose (no HIP, no other header of the library): vt_sketchsearch.h uses
// it, and tests/sketch6_query_check.cpp and tests/sketch6_split_check.cpp build it with plain g++ under AddressSanitizer
// and UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace vt_host {

constexpr int kSketch6Levels = 3;  // J: q = sum_j t_j Q_j + eta, |Q_j| <= 7
constexpr uint32_t sketch6_ld8(uint32_t d) { return (d + 127) / 128 * 128; }
// dwords of one level's nibble image: eight elements per dword, nibble i of dword g is element 8 g + i
constexpr uint32_t sketch6_level_words(uint32_t d) { return sketch6_ld8(d) / 8; }

// The query in J signed-nibble levels.  Level j's integers are chosen with a reciprocal from the residual the levels
// before it left; the residual is then re-formed from the chosen integers in f64 (t Q has at most 27 significant bits:
// exact), so q - sum_j t_j Q_j = eta holds for any |Q| <= 7 and only the bound's tightness depends on the rounding.
// img: [J][sketch6_level_words(d)] dwords; resid: d doubles of scratch, eta on return; t: J scales; *ee = sum eta_i^2.
inline void sketch6_query_levels(const float *q, uint32_t d, uint32_t *img, double *resid, float *t, double *ee) {
  const uint32_t lw = sketch6_level_words(d);
  std::memset(img, 0, (size_t)kSketch6Levels * lw * sizeof(uint32_t));
  constexpr double kRound = 0x1.8p52;  // (v + kRound) - kRound: v to the nearest integer, |v| < 2^51, no library call
  for (uint32_t i = 0; i < d; ++i) resid[i] = (double)q[i];
  for (int j = 0; j < kSketch6Levels; ++j) {
    double m = 0.0;
    for (uint32_t i = 0; i < d; ++i) m = std::max(m, std::fabs(resid[i]));
    float tj = (float)(m / 7.0);
    if (!(tj > 0.0f) || !std::isfinite(tj) || !std::isfinite(7.0 / (double)tj)) tj = 0.0f;
    t[j] = tj;
    const double td = (double)tj, inv = tj > 0.0f ? 1.0 / td : 0.0;
    uint32_t *lv = img + (size_t)j * lw;
    for (uint32_t i = 0; i < d; ++i) {
      const double r = resid[i];
      const int v = r == r ? (int)std::max(-7.0, std::min(7.0, (r * inv + kRound) - kRound)) : 0;
      lv[i >> 3] |= ((uint32_t)v & 0xfu) << (4 * (i & 7));
      resid[i] = r - td * v;
    }
  }
  double s = 0.0;
  for (uint32_t i = 0; i < d; ++i) s += resid[i] * resid[i];
  *ee = s;
}

// What the pass needs to bound a level it keeps off the L plane (0 <= L_i <= 3): over one level's nibble image
// (lw dwords, sketch6_query_levels' layout; padding nibbles are 0), *pos = the sum of its positive entries, *neg = the sum
// of its negative entries (<= 0), *l1 = sum |Q_i| = *pos - *neg.  Q.L then lies in [3 *neg, 3 *pos].
inline void sketch6_level_sums(const uint32_t *level, uint32_t lw, int64_t *pos, int64_t *neg, int64_t *l1) {
  int64_t p = 0, n = 0;
  for (uint32_t g = 0; g < lw; ++g) {
    const uint32_t w = level[g];
    for (int i = 0; i < 8; ++i) {
      const int nib = (int)((w >> (4 * i)) & 0xfu);
      const int v = nib >= 8 ? nib - 16 : nib;  // (the signed nibble)
      if (v > 0) p += v;
      else n += v;
    }
  }
  *pos = p;
  *neg = n;
  *l1 = p - n;
}

// The bound itself, for the pass: the last level stays off the L plane, and its share there is *c -+ *w per unit of s_r with
// *c = 1.5 t (*pos + *neg) and *w = 1.5 t ||Q||_1 (the middle of [3 *neg, 3 *pos] and half its width; exact: 25 bits times 19).
inline void sketch6_level_bound(const uint32_t *level, uint32_t lw, float t, double *c, double *w) {
  int64_t pos = 0, neg = 0, l1 = 0;
  sketch6_level_sums(level, lw, &pos, &neg, &l1);
  const double t3 = 1.5 * (double)t;
  *c = t3 * (double)(pos + neg);
  *w = t3 * (double)l1;
}

// The row quantiser as nibble_row (vt_sketch_nibble.cuh) has it: s = max|x| / 31 in f32, X = round(x * (31 / max|x|)) clamped
// to [-31, 31]; X = 4 H + L with H = X >> 2 in [-8, 7] and L = X & 3.  rho >= ||x - s X|| and nu >= s ||X||, from f64
// sums with a 2^-30 margin, rounded up to f32.  (The device sums in another order: its bounds may differ in the last bits.)
inline void sketch6_quantise_row(const float *x, uint32_t d, int8_t *X, float *s_out, float *rho_out, float *nu_out) {
  float m = 0.0f;
  for (uint32_t i = 0; i < d; ++i) m = std::max(m, std::fabs(x[i]));
  float s = m / 31.0f;
  const float inv = 31.0f / m;
  const bool quantise = m > 0.0f && std::isfinite(inv) && s > 0.0f;
  if (!quantise) s = 0.0f;
  double res = 0.0, xx = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    int v = 0;
    if (quantise) {
      v = (int)std::nearbyint(x[i] * inv);
      v = v > 31 ? 31 : (v < -31 ? -31 : v);
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

}  // namespace vt_host

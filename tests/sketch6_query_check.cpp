// The host side of the 6-bit sketch (vettore_amd/csrc/host/vt_sketch6.h) is plain C++: built here with g++ under
// AddressSanitizer and UBSan.  The query's nibble levels must be signed nibbles |Q_j| <= 7 with zero padding, and
// q - sum_j t_j Q_j, recomputed here in f64, must be the eta the bound is given; the row quantiser must satisfy
// X = 4 H + L with its rho and nu above the sums recomputed here.  The bound of the level kept off the L plane (c3, w3)
// must be 1.5 t (P + N) and 1.5 t ||Q||_1 of sums formed here from the integers the level was packed from.
#include "../vettore_amd/csrc/host/vt_sketch6.h"

#include <cfloat>
#include <cstdio>
#include <random>
#include <vector>

using namespace vt_host;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++failures;                                         \
    }                                                     \
  } while (0)

static int nibble(const uint32_t *level, uint32_t i) {
  const int v = (int)((level[i >> 3] >> (4 * (i & 7))) & 0xfu);
  return v >= 8 ? v - 16 : v;
}

static void check_query(const std::vector<float> &q, const char *name) {
  const uint32_t d = (uint32_t)q.size(), lw = sketch6_level_words(d);
  // exact-size heap blocks: a write past either end is AddressSanitizer's to report
  std::vector<uint32_t> img((size_t)kSketch6Levels * lw, 0xffffffffu);
  std::vector<double> resid(d, -1.0);
  float t[kSketch6Levels];
  double ee = -1.0;
  sketch6_query_levels(q.data(), d, img.data(), resid.data(), t, &ee);
  double ee2 = 0.0, qmax = 0.0;
  for (uint32_t i = 0; i < d; ++i) qmax = std::max(qmax, std::fabs((double)q[i]));
  for (uint32_t i = 0; i < d; ++i) {
    double rest = (double)q[i];
    for (int j = 0; j < kSketch6Levels; ++j) {
      const int v = nibble(img.data() + (size_t)j * lw, i);
      CHECK(v >= -7 && v <= 7, "%s: level %d element %u is %d", name, j, i, v);
      rest -= (double)t[j] * v;
    }
    CHECK(std::fabs(rest - resid[i]) <= qmax * 0x1p-48, "%s: eta[%u] %.17g, recomputed %.17g", name, i, resid[i], rest);
    ee2 += rest * rest;
  }
  CHECK(std::fabs(ee - ee2) <= ee2 * 1e-9 + qmax * qmax * 0x1p-90, "%s: sum eta^2 %.17g, recomputed %.17g", name, ee, ee2);
  for (int j = 0; j < kSketch6Levels; ++j) {
    CHECK(std::isfinite(t[j]) && t[j] >= 0.0f, "%s: t[%d] = %g", name, j, (double)t[j]);
    for (uint32_t i = d; i < lw * 8; ++i) CHECK(nibble(img.data() + (size_t)j * lw, i) == 0, "%s: padding %u of level %d", name, i, j);
  }
  // a level leaves at most t_j / 2 = (its input's maximum) / 14 per coordinate (unless a scale underflowed to nothing)
  if (t[kSketch6Levels - 1] > 0.0f)
    for (uint32_t i = 0; i < d; ++i) CHECK(std::fabs(resid[i]) <= qmax / (14.0 * 14 * 14) * (1 + 1e-6), "%s: eta[%u] = %g", name, i, resid[i]);
}

static void check_row(const std::vector<float> &x, const char *name) {
  const uint32_t d = (uint32_t)x.size();
  std::vector<int8_t> X(d, 99);
  float s = -1, rho = -1, nu = -1;
  sketch6_quantise_row(x.data(), d, X.data(), &s, &rho, &nu);
  double res = 0.0, xx = 0.0;
  for (uint32_t i = 0; i < d; ++i) {
    const int v = X[i], H = v >> 2, L = v & 3;
    CHECK(v >= -31 && v <= 31 && H >= -8 && H <= 7 && L >= 0 && L <= 3 && 4 * H + L == v, "%s: X[%u] = %d", name, i, v);
    const double r = (double)x[i] - (double)s * v;
    res += r * r;
    xx += (double)v * v;
  }
  CHECK((double)rho >= std::sqrt(res) && (double)nu >= (double)s * std::sqrt(xx), "%s: rho %g nu %g", name, (double)rho, (double)nu);
  CHECK(std::isfinite(rho) && std::isfinite(nu) && s >= 0.0f, "%s: s %g", name, (double)s);
}

// One level of d signed nibbles (`zero`: all of them 0; else mixed signs), packed here as sketch6_query_levels packs them.
static void check_level_bound(uint32_t d, bool zero, float t, std::mt19937 &rng) {
  const uint32_t lw = sketch6_level_words(d);
  std::vector<uint32_t> level(lw, 0u);  // exact-size: a read past its end is AddressSanitizer's to report
  std::uniform_int_distribution<int> pick(-7, 7);
  long long pos = 0, neg = 0, l1 = 0;
  for (uint32_t i = 0; i < d; ++i) {
    const int v = zero ? 0 : (i == 0 ? 7 : i == 1 ? -7 : pick(rng));  // (both signs are there whatever the draw)
    level[i >> 3] |= ((uint32_t)v & 0xfu) << (4 * (i & 7));
    if (v > 0) pos += v;
    if (v < 0) neg += v;
    l1 += v < 0 ? -v : v;
  }
  double c = -1.0, w = -1.0;
  sketch6_level_bound(level.data(), lw, t, &c, &w);
  // (integers below 2^13 times a 24-bit scale times 1.5: every product is exact in f64, so the sums must agree to the bit)
  const double want_c = 1.5 * (double)t * (double)(pos + neg), want_w = 1.5 * (double)t * (double)l1;
  CHECK(c == want_c && w == want_w, "level bound d=%u zero=%d: c %.17g (want %.17g), w %.17g (want %.17g)", d, (int)zero, c, want_c, w, want_w);
  CHECK(w >= std::fabs(c), "level bound d=%u: |c| %.17g above w %.17g", d, c, w);
  if (zero) CHECK(c == 0.0 && w == 0.0, "level bound d=%u of a zero level: c %.17g w %.17g", d, c, w);
}

int main() {
  std::mt19937 rng(20260722);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  for (uint32_t d : {129u, 256u}) {  // off and on the 128 grid
    check_level_bound(d, false, 0.0123f, rng);
    check_level_bound(d, true, 0.0123f, rng);
  }
  for (uint32_t d : {1u, 7u, 8u, 31u, 33u, 129u, 192u, 257u, 768u, 1001u}) {
    std::vector<float> q(d);
    for (auto &v : q) v = u(rng);
    check_query(q, "uniform");
    check_row(q, "uniform");
    std::vector<float> z(d, 0.0f);
    check_query(z, "zeros");
    check_row(z, "zeros");
    std::vector<float> sub(d);
    for (uint32_t i = 0; i < d; ++i) sub[i] = (float)((int)(i % 5) - 2) * FLT_TRUE_MIN;  // subnormals
    check_query(sub, "subnormals");
    check_row(sub, "subnormals");
    std::vector<float> big = q;
    big[d / 2] = 3e38f;  // one huge coordinate
    check_query(big, "one huge coordinate");
    check_row(big, "one huge coordinate");
    std::vector<float> one(d, 0.0f);
    one[d - 1] = -0.25f;
    check_query(one, "one non-zero coordinate");
    check_row(one, "one non-zero coordinate");
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}

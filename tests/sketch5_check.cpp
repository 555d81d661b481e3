// tests/sketch5_check.cpp -- host/vt_sketch5.h against naive recounts: the row quantiser (ranges, X = 2 H + L, rho and nu as
// upper bounds) and the bound of the query level kept off the one-bit L plane (for every L in {0, 1}^d tried, Q.L lies in
// c -+ w).  Built by tests/test_sketch5_host.py with g++ under AddressSanitizer and UBSan.  Prints "ok".
#include "../vettore_amd/csrc/host/vt_sketch5.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace vt_host;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("line %d: %s\n", __LINE__, #c);                  \
      if (++fails > 20) std::exit(1);                              \
    }                                                              \
  } while (0)

static int nibble(const uint32_t *level, uint32_t i) {
  const int nib = (int)((level[i >> 3] >> (4 * (i & 7))) & 0xfu);
  return nib >= 8 ? nib - 16 : nib;
}

static void check_row(const std::vector<float> &x) {
  const uint32_t d = (uint32_t)x.size();
  std::vector<int8_t> X(d, 99), H(d, 99);
  std::vector<uint8_t> L(d, 99);
  float s = -1.f, rho = -1.f, nu = -1.f;
  sketch5_quantise_row(x.data(), d, X.data(), &s, &rho, &nu);
  sketch5_split(X.data(), d, H.data(), L.data());
  float m = 0.f;
  for (float v : x) m = std::max(m, std::fabs(v));
  CHECK(s >= 0.f && (m > 0.f ? s == m / 15.0f || s == 0.f : s == 0.f));
  long double res = 0, xx = 0;
  int peak = 0;
  for (uint32_t i = 0; i < d; ++i) {
    CHECK(X[i] >= -15 && X[i] <= 15);
    CHECK(H[i] >= -8 && H[i] <= 7 && L[i] <= 1 && 2 * H[i] + L[i] == X[i]);
    peak = std::max(peak, std::abs((int)X[i]));
    const long double r = (long double)x[i] - (long double)s * X[i];
    res += r * r;
    xx += (long double)X[i] * X[i];
  }
  if (s > 0.f) CHECK(peak == 15);
  CHECK((long double)rho >= sqrtl(res) && (long double)nu >= (long double)s * sqrtl(xx));
  CHECK((long double)rho <= sqrtl(res) * (1 + 1e-6L) + 1e-44L && (long double)nu <= (long double)s * sqrtl(xx) * (1 + 1e-6L) + 1e-44L);
}

int main() {
  std::mt19937 rng(12345);
  std::uniform_real_distribution<float> uni(-1.f, 1.f);
  CHECK(sketch5_runs(129) == 11 && sketch5_runs(256) == 11 && sketch5_runs(768) == 31 && sketch5_runs(1) == 6);
  for (uint32_t d : {1u, 7u, 128u, 129u, 200u, 768u, 1000u}) {
    std::vector<float> x(d);
    for (int rep = 0; rep < 6; ++rep) {
      for (auto &v : x) v = uni(rng);
      if (rep == 1) x[d / 2] = 1000.f;                       // one huge coordinate
      if (rep == 2) for (auto &v : x) v = 0.f;               // a zero row
      if (rep == 3) for (auto &v : x) v = v < 0 ? -3.f : 3.f;  // +-max only
      if (rep == 4) for (auto &v : x) v *= 1e-38f;           // subnormal products
      if (rep == 5) for (auto &v : x) v *= 1e37f;
      check_row(x);
    }
    // the level bound against a recount from the nibbles, and against Q.L itself for random and extreme L
    const uint32_t lw = sketch6_level_words(d);
    std::vector<uint32_t> img((size_t)kSketch6Levels * lw, 0xdeadbeefu);
    std::vector<double> resid(d);
    float t[kSketch6Levels];
    double ee = 0;
    for (int rep = 0; rep < 4; ++rep) {
      for (auto &v : x) v = rep == 3 ? 0.f : uni(rng) * (rep == 2 ? 1e-20f : 1.f);
      sketch6_query_levels(x.data(), d, img.data(), resid.data(), t, &ee);
      for (int j = 0; j < kSketch6Levels; ++j) {
        const uint32_t *level = img.data() + (size_t)j * lw;
        long pos = 0, neg = 0;
        for (uint32_t i = 0; i < 8 * lw; ++i) {
          const int v = nibble(level, i);
          CHECK(v >= -7 && v <= 7 && (i < d || v == 0));
          (v > 0 ? pos : neg) += v;
        }
        double c = -1, w = -1;
        sketch5_level_bound(level, lw, t[j], &c, &w);
        CHECK(c == 0.5 * (double)t[j] * (double)(pos + neg) && w == 0.5 * (double)t[j] * (double)(pos - neg));
        for (int trial = 0; trial < 8; ++trial) {
          long ql = 0;
          for (uint32_t i = 0; i < d; ++i) {
            const int v = nibble(level, i);
            const int l = trial == 0 ? (v > 0) : trial == 1 ? (v < 0) : (int)(rng() & 1u);
            ql += v * l;
          }
          const double share = (double)t[j] * (double)ql;  // exact: 24 bits times 20
          CHECK(share >= c - w && share <= c + w);
          if (trial == 0) CHECK(share == c + w);
          if (trial == 1) CHECK(share == c - w);
        }
      }
    }
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}

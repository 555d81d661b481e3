// tests/sketch6_split_check.cpp -- host/vt_sketch6.h's sketch6_level_sums against a naive recount from the nibbles, built
// by tests/test_sketch6_split.py with g++ under AddressSanitizer and UBSan.  Prints "ok".
#include "../vettore_amd/csrc/host/vt_sketch6.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace vt_host;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static int nibble(const uint32_t *level, uint32_t i) {
  const int nib = (int)((level[i >> 3] >> (4 * (i & 7))) & 0xfu);
  return nib >= 8 ? nib - 16 : nib;
}

// every level of q's image: the sums equal a recount element by element, and the padding contributes nothing
static const uint32_t *check_query(const std::vector<float> &q, std::vector<uint32_t> &img) {
  const uint32_t d = (uint32_t)q.size(), lw = sketch6_level_words(d);
  img.assign((size_t)kSketch6Levels * lw, 0xdeadbeefu);
  std::vector<double> resid(d);
  float t[kSketch6Levels];
  double ee = 0.0;
  sketch6_query_levels(q.data(), d, img.data(), resid.data(), t, &ee);
  for (int j = 0; j < kSketch6Levels; ++j) {
    const uint32_t *level = img.data() + (size_t)j * lw;
    int64_t pos = 0, neg = 0, l1 = 0;
    for (uint32_t i = 0; i < d; ++i) {
      const int v = nibble(level, i);
      CHECK(v >= -7 && v <= 7);
      if (v > 0) pos += v;
      if (v < 0) neg += v;
      l1 += std::abs(v);
    }
    for (uint32_t i = d; i < 8 * lw; ++i) CHECK(nibble(level, i) == 0);
    int64_t gp = -1, gn = 1, gl = -1;
    sketch6_level_sums(level, lw, &gp, &gn, &gl);
    CHECK(gp == pos && gn == neg && gl == l1);
    CHECK(gp >= 0 && gn <= 0 && gl == gp - gn);
  }
  return img.data() + (size_t)(kSketch6Levels - 1) * lw;
}

int main() {
  std::mt19937 rng(20260721);
  std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
  for (uint32_t d : {129u, 192u, 257u, 768u, 1000u}) {
    std::vector<uint32_t> img;
    std::vector<float> q(d);
    for (auto &v : q) v = uni(rng);
    check_query(q, img);
    for (uint32_t hot : {0u, d / 3, d - 1}) {
      std::vector<float> one(d, 0.0f);
      one[hot] = hot & 1 ? -2.5f : 1.0f;
      const uint32_t *last = check_query(one, img);
      int64_t p = 0, n = 0, l = 0;
      sketch6_level_sums(last, sketch6_level_words(d), &p, &n, &l);
      CHECK(l <= 7);  // (one element at most is not zero)
    }
    {
      std::vector<float> zero(d, 0.0f);
      const uint32_t *last = check_query(zero, img);
      int64_t p = 1, n = 1, l = 1;
      sketch6_level_sums(last, sketch6_level_words(d), &p, &n, &l);
      CHECK(p == 0 && n == 0 && l == 0);
    }
    // a query whose third level is +7 everywhere: a constant vector leaves every level one residual, the same in every
    // coordinate, and its sign is the rounding's; the first constant whose second residual is positive serves
    bool found = false;
    for (int k = 1; k <= 400 && !found; ++k) {
      std::vector<float> c(d, 0.37f * (float)k + 0.011f);
      const uint32_t *last = check_query(c, img);
      bool all7 = true;
      for (uint32_t i = 0; i < d; ++i) all7 = all7 && nibble(last, i) == 7;
      if (!all7) continue;
      found = true;
      int64_t p = 0, n = 0, l = 0;
      sketch6_level_sums(last, sketch6_level_words(d), &p, &n, &l);
      CHECK(p == 7 * (int64_t)d && n == 0 && l == 7 * (int64_t)d);
    }
    CHECK(found);
    // and the image itself, whatever query would give it: every nibble -7, then +7 with the padding left zero
    const uint32_t lw = sketch6_level_words(d);
    std::vector<uint32_t> level(lw, 0u);
    for (uint32_t i = 0; i < d; ++i) level[i >> 3] |= 0x9u << (4 * (i & 7));
    int64_t p = 0, n = 0, l = 0;
    sketch6_level_sums(level.data(), lw, &p, &n, &l);
    CHECK(p == 0 && n == -7 * (int64_t)d && l == 7 * (int64_t)d);
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}

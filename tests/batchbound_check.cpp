// batchbound_check.cpp -- host/vt_batchbound.h on the CPU (tests/test_batch_model.py builds this with g++ under
// AddressSanitizer and UBSan and runs it).  Checks what the header promises about itself -- the three bf16 terms add up to
// the margin to a few units in the last place, the margin grows with every argument, the guard sits at 1e18 -- and prints
// the margin and its terms on a grid of arguments as hex floats, one line each, for the test to hold against the model's
// own derivation (tests/batch_ref.py).  The last line is "ok".
#include "../vettore_amd/csrc/host/vt_batchbound.h"

#include <cstdio>
#include <limits>

int main() {
  const uint32_t dims[] = {1, 3, 64, 100, 192, 320, 768, 4096};
  const double mags[] = {0.0, 1e-30, 1e-20, 0.37, 1.0, 27.5, 1e15, 9.9e17};
  int bad = 0;
  for (int l2 = 0; l2 < 2; ++l2)
    for (uint32_t d : dims)
      for (double qn : mags)
        for (double xn : mags) {
          const vt_host::BatchBf16Terms t = vt_host::batch_bf16_terms(l2 != 0, d, qn, xn);
          const double e16 = vt_host::batch_eps(l2 != 0, true, d, qn, xn), e32 = vt_host::batch_eps(l2 != 0, false, d, qn, xn);
          const double sum = t.rounding + t.accumulation + t.flush;
          if (!(std::fabs(sum - e16) <= 8.0 * std::numeric_limits<double>::epsilon() * e16)) {
            std::fprintf(stderr, "terms do not add up: l2 %d d %u qn %g xn %g: %a against %a\n", l2, d, qn, xn, sum, e16);
            ++bad;
          }
          if (!(t.rounding >= 0 && t.accumulation >= 0 && t.flush >= 0 && e32 >= 0 && e16 >= e32 && std::isfinite(e16))) {
            std::fprintf(stderr, "signs / order: l2 %d d %u qn %g xn %g\n", l2, d, qn, xn);
            ++bad;
          }
          // larger arguments never shrink the margin
          if (!(vt_host::batch_eps(l2 != 0, true, d + 1, qn, xn) >= e16 && vt_host::batch_eps(l2 != 0, true, d, qn * 1.5, xn) >= e16 &&
                vt_host::batch_eps(l2 != 0, true, d, qn, xn * 1.5) >= e16 && vt_host::batch_eps(l2 != 0, false, d + 1, qn, xn) >= e32 &&
                vt_host::batch_eps(l2 != 0, false, d, qn * 1.5, xn) >= e32 && vt_host::batch_eps(l2 != 0, false, d, qn, xn * 1.5) >= e32)) {
            std::fprintf(stderr, "not monotone: l2 %d d %u qn %g xn %g\n", l2, d, qn, xn);
            ++bad;
          }
          std::printf("%d %u %a %a %a %a %a %a %a\n", l2, d, qn, xn, e32, e16, t.rounding, t.accumulation, t.flush);
        }
  // the guard: K2 always, K2b / K2s strictly below 1e18 on both sides
  const bool guard = vt_host::batch_magnitudes_ok(false, 1e30, 1e30) && vt_host::batch_magnitudes_ok(true, 9.9e17, 9.9e17) &&
                     !vt_host::batch_magnitudes_ok(true, 1e18, 1.0) && !vt_host::batch_magnitudes_ok(true, 1.0, 1e18) &&
                     !vt_host::batch_magnitudes_ok(true, std::numeric_limits<double>::quiet_NaN(), 1.0) &&
                     !vt_host::batch_magnitudes_ok(true, 1.0, std::numeric_limits<double>::infinity());
  if (!guard) {
    std::fprintf(stderr, "guard\n");
    ++bad;
  }
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}

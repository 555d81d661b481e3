// vt_batchbound.h -- the margin of the matrix-core groups' certificate (K2 / K2b / K2s) as one function.
// Plain C++ with no dependency but <cmath>: host/vt_batch.h (batch_group_finish) judges with it, tests/batch_probe.cpp
// exports it to the kernel tests and tests/batchbound_check.cpp checks it on the CPU, so nobody retypes the formula.
//
// A nomination pass forms, per (query q, row x), the score s = q.x (dot family) or s = 2 q.x - |x|^2 (L2 family).  With
// u = 2^-24, d the row length, |q| the query's norm and X the largest row norm, batch_eps bounds |s - s_ref| where s_ref
// is the same score in the reference's own f32 arithmetic:
//   K2 (f32 operands): both sums are d-term f32 sums of the same products:
//     dot family   2.5 d u |q| X              (2 gamma_d |q| X, rounded up)
//     L2 family    3.5 d u (|q| + X)^2
//   K2b / K2s (operands rounded to bf16 first, 8 significant bits, round to nearest even: relative error <= ub = 2^-8
//   each), three terms -- batch_bf16_terms names them one by one:
//     rounding       every product carries a relative error of at most 2 ub + ub^2 and, by Cauchy-Schwarz, the sum an
//                    absolute one of at most (2 ub + ub^2) |q| X; twice that for the L2 family's 2 q.x
//     accumulation   the bf16 products are exact in f32; the matrix core's f32 accumulation of them is priced generously,
//                    together with the reference's own summation error, whatever the order and the rounding of the
//                    partial sums: 8 d u |q| X, or 8 d u (|q| + X)^2 for the L2 family (the norm's rounding included)
//     flush          subnormal operands may be flushed: at most 2^-126 per element times the other operand,
//                    sqrt(d) 2^-126 (|q| + X) over a row; priced at 2^-120 sqrt(d) (|q| + X)
// Rounding to bf16 can overflow only near f32's largest values: batch_magnitudes_ok is the guard under which the bf16 margin
// is valid at all.
#pragma once

#include <cmath>
#include <cstdint>

namespace vt_host {

struct BatchBf16Terms {
  double rounding, accumulation, flush;
};

inline BatchBf16Terms batch_bf16_terms(bool l2_family, uint32_t d, double qnorm, double xnorm) {
  const double u = std::ldexp(1.0, -24), ub = std::ldexp(1.0, -8);
  BatchBf16Terms t;
  t.flush = std::ldexp(1.0, -120) * std::sqrt((double)d) * (qnorm + xnorm);
  if (l2_family) {
    t.rounding = 2.0 * (2.0 * ub + ub * ub) * qnorm * xnorm;
    t.accumulation = 8.0 * (double)d * u * (qnorm + xnorm) * (qnorm + xnorm);
  } else {
    t.rounding = (2.0 * ub + ub * ub) * qnorm * xnorm;
    t.accumulation = 8.0 * (double)d * u * qnorm * xnorm;
  }
  return t;
}

// The whole margin.  (The bf16 forms are the three terms above written as one expression, in the order the certificate
// has always evaluated them: the sum of batch_bf16_terms agrees with it to a few units in the last place, not bit for bit.)
inline double batch_eps(bool l2_family, bool bf16, uint32_t d, double qnorm, double xnorm) {
  const double u = std::ldexp(1.0, -24), ub = std::ldexp(1.0, -8);
  if (l2_family) {
    double eps = 3.5 * (double)d * u * (qnorm + xnorm) * (qnorm + xnorm);
    if (bf16)
      eps = 2.0 * (2.0 * ub + ub * ub) * qnorm * xnorm + 8.0 * (double)d * u * (qnorm + xnorm) * (qnorm + xnorm) +
            std::ldexp(1.0, -120) * std::sqrt((double)d) * (qnorm + xnorm);
    return eps;
  }
  double eps = 2.5 * (double)d * u * qnorm * xnorm;
  if (bf16)
    eps = (2.0 * ub + ub * ub + 8.0 * (double)d * u) * qnorm * xnorm +
          std::ldexp(1.0, -120) * std::sqrt((double)d) * (qnorm + xnorm);
  return eps;
}

// K2b / K2s certify only below these magnitudes (no operand's rounding to bf16 overflows, no margin is infinite)
inline bool batch_magnitudes_ok(bool bf16, double qnorm, double xnorm) { return !bf16 || (qnorm < 1e18 && xnorm < 1e18); }

}  // namespace vt_host

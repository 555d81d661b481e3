// vt_pair.cuh -- the score of a (vector, vector) pair when ONE lane walks the pair from start to finish, so that the
// reference's order needs no cross-lane exchange: the arithmetic of K9 (vt_maxsim.hip), K9r and K9rb (vt_maxsim_pair.cuh),
// K11 (vt_hnsw.hip) and K12 (vt_mmr.hip), stated here once.
//   * the f32 families (OP_DOT / OP_L2 / OP_L1 / OP_LINF): per 8-float chunk eight separately rounded element operations
//     (elem), the chunk folded in the selected lane order (chunk_sum1), `acc = comb(acc, chunk)` in chunk order, then the
//     scalar tail -- K1's arithmetic, one lane wide -- and compute()'s finish with the f64 recovery of a non-finite
//     value, returned by value (f32_raws, finish_raw);
//   * cosine (PAIR_COS): the f64 dot, sequentially, over the two vectors' f64 norms (cosine_dots, cosine_raw);
//   * Hamming and Jaccard (PAIR_COUNT): integer counts over truthiness -- no 4096 trick, any d is exact (count_raws).
// A raw value that is NaN means "metric overflow".  A lane walks K vectors against one row at once: the row's chunk is
// loaded once for K chains (K = 8: MaxSim's query vectors; K = 1: K11, K12).
// The kernels keep their own loops, staging and reductions; their launchers pick the instance with dispatch_pair.
#pragma once
#include <type_traits>

#include "vt_scan.cuh"

namespace vt {
namespace dev {

namespace {

constexpr int kQB = 8;                    // vectors per lane pass of the 8-wide callers (MaxSim's query vectors)
enum { PAIR_COS = 6, PAIR_COUNT = 7 };    // the two families beside OP_DOT / OP_L2 / OP_L1 / OP_LINF

// compute() (distances.rs:42-68) after the f32 chain: the metric's finish, then the f64 recovery of a non-finite value.
template <int OP>
__device__ __forceinline__ float finish_raw(int metric, float acc, const float *q, const float *x, uint32_t d) {
  float raw = acc;
  if (metric == M_NIP) raw = -acc;
  else if (metric == M_L2) raw = finite_f32(acc) ? __builtin_sqrtf(acc) : acc;
  if (!finite_f32(raw)) raw = recover_overflow(metric, q, x, d);
  return raw;
}

// similarity_value (distances.rs:122-128)
__device__ __forceinline__ float similarity(int metric, float raw) {
  if (metric == M_COS || metric == M_IP) return raw;
  if (metric == M_NIP) return -raw;
  return 1.0f / (1.0f + raw);
}

// raw[k] = compute() of (v[k], row) in an f32 family: the chain, then its finish.  ROW_LEFT: the row is the left operand
// (K11: the stored row).  ROW_SCALAR: the row's chunk is read as eight scalars -- for a row that is not 16-byte aligned
// (K9: its stride is only >= d); otherwise as two 16-byte loads.  The vectors v[k] are 16-byte aligned; only whole chunks
// are read 16 bytes at a time.
// (The finish belongs in here: with the accumulators handed back to the caller between chain and finish, several 8-wide
// instances came out of the register allocator an occupancy class lower -- profiles/pair_chain/resources.txt.)
template <int OP, int ORDER, int K, bool ROW_LEFT, bool ROW_SCALAR>
__device__ __forceinline__ void f32_raws(int metric, const float *const (&v)[K], const float *row, uint32_t d,
                                         float (&raw)[K]) {
  const uint32_t cfull = d / 8;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0f;
  for (uint32_t c = 0; c < cfull; ++c) {
    float r[8];
    if (ROW_SCALAR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = row[c * 8 + e];
    } else {
      const f32x4 ra = *reinterpret_cast<const f32x4 *>(row + c * 8);
      const f32x4 rb = *reinterpret_cast<const f32x4 *>(row + c * 8 + 4);
      r[0] = ra.x, r[1] = ra.y, r[2] = ra.z, r[3] = ra.w, r[4] = rb.x, r[5] = rb.y, r[6] = rb.z, r[7] = rb.w;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const f32x4 va = *reinterpret_cast<const f32x4 *>(v[k] + c * 8);
      const f32x4 vb = *reinterpret_cast<const f32x4 *>(v[k] + c * 8 + 4);
      const float q[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
      float l[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) l[e] = ROW_LEFT ? elem<OP>(0, r[e], q[e]) : elem<OP>(0, q[e], r[e]);
      acc[k] = comb<OP>(0, acc[k], chunk_sum1<OP, ORDER>(l));
    }
  }
  for (uint32_t e = cfull * 8; e < d; ++e) {  // the scalar tail, one element at a time (never a row's pad)
    const float re = row[e];
#pragma unroll
    for (int k = 0; k < K; ++k)
      acc[k] = comb<OP>(0, acc[k], ROW_LEFT ? elem<OP>(0, re, v[k][e]) : elem<OP>(0, v[k][e], re));
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    raw[k] = ROW_LEFT ? finish_raw<OP>(metric, acc[k], row, v[k], d) : finish_raw<OP>(metric, acc[k], v[k], row, d);
}

// cosine() (distances.rs:160-185) of (v[k], row) in two steps, so that a caller reads the norms between them and holds
// none across the dot.  dot[k]: the f64 dot, sequentially -- fma(q, x, acc) == acc + q*x, a product of two f32 is exact in
// f64.
template <int K>
__device__ __forceinline__ void cosine_dots(const float *const (&v)[K], const float *row, uint32_t d, double (&dot)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) dot[k] = 0.0;
  for (uint32_t e = 0; e < d; ++e) {
    const double xv = (double)row[e];
#pragma unroll
    for (int k = 0; k < K; ++k) dot[k] = __builtin_fma((double)v[k][e], xv, dot[k]);
  }
}
// ... and the raw value from the dot and the two vectors' f64 norms: cosine_raw (vt_scan.cuh)

// raw[k] = hamming() / jaccard() (distances.rs:319-347) of (v[k], row) over truthiness
template <int K>
__device__ __forceinline__ void count_raws(int metric, const float *const (&v)[K], const float *row, uint32_t d,
                                           float (&raw)[K]) {
  uint32_t ham[K], inter[K], uni[K];
#pragma unroll
  for (int k = 0; k < K; ++k) ham[k] = inter[k] = uni[k] = 0;
  for (uint32_t e = 0; e < d; ++e) {
    const bool xr = row[e] != 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool ql = v[k][e] != 0.0f;
      ham[k] += ql != xr;
      inter[k] += ql && xr;
      uni[k] += ql || xr;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (metric == M_HAM) raw[k] = (float)ham[k];
    else raw[k] = uni[k] == 0 ? 0.0f : 1.0f - (float)inter[k] / (float)uni[k];
  }
}

// ---- host side: from (metric, order) to an instance ------------------------------------------------------------------
// The families a kernel is built for, one bit per OP; kPairCosAsDot: cosine runs the dot instance (K11 ranks by it).
constexpr unsigned kPairF32 = 1u << OP_DOT | 1u << OP_L2 | 1u << OP_L1 | 1u << OP_LINF;
constexpr unsigned kPairCos = 1u << PAIR_COS, kPairCount = 1u << PAIR_COUNT, kPairCosAsDot = 1u << 8;

template <unsigned FAMILIES, int OP, class F>
hipError_t pair_instance(int order, F &f) {
  using std::integral_constant;
  if constexpr (!(FAMILIES & 1u << OP)) return hipErrorInvalidValue;
  else if constexpr (OP >= PAIR_COS) return f(integral_constant<int, OP>{}, integral_constant<int, 0>{});  // (no lane order)
  else switch (order) {
    case 0: return f(integral_constant<int, OP>{}, integral_constant<int, 0>{});
    case 1: return f(integral_constant<int, OP>{}, integral_constant<int, 1>{});
    case 2: return f(integral_constant<int, OP>{}, integral_constant<int, 2>{});
    default: return f(integral_constant<int, OP>{}, integral_constant<int, 3>{});
  }
}

// f(op, order) with op() and order() compile-time constants, for the instance that serves `metric` in lane order `order`;
// hipErrorInvalidValue for a metric whose family the caller's kernel does not have.
template <unsigned FAMILIES, class F>
hipError_t dispatch_pair(int metric, int order, F f) {
  switch (metric) {
    case M_COS: return pair_instance<FAMILIES, (FAMILIES & kPairCosAsDot) ? OP_DOT : PAIR_COS>(order, f);
    case M_HAM:
    case M_JAC: return pair_instance<FAMILIES, PAIR_COUNT>(order, f);
    case M_IP:
    case M_NIP: return pair_instance<FAMILIES, OP_DOT>(order, f);
    case M_L2:
    case M_L2SQ: return pair_instance<FAMILIES, OP_L2>(order, f);
    case M_L1: return pair_instance<FAMILIES, OP_L1>(order, f);
    case M_LINF: return pair_instance<FAMILIES, OP_LINF>(order, f);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

}  // namespace dev
}  // namespace vt

// vt_maxsim_pair.cuh -- what K9r (vt_maxsim_resident.hip) and K9rb (vt_maxsim_batch.hip) share: one wave's pass over one
// document of a resident store for the eight query vectors of each of its lanes.  A lane is (row of the tile, group of
// eight query vectors); the document's rows come through the wave's LDS tile, `tt` at a time, and every (query vector,
// document vector) pair is one lane's own chain in the reference's order (K9's arithmetic, vt_maxsim.hip).  The two
// kernels differ only in where a lane's eight query vectors come from and in what they do with the maxima.
#pragma once
#include "vt_scan.cuh"

namespace vt {
namespace dev {

namespace {

constexpr int kQB = 8;                       // query vectors per lane pass (as in K9)
constexpr size_t kResidentLds = 128 * 1024;  // LDS of a block: the query panel and four tiles
enum { MS_COS = 6, MS_COUNT = 7 };           // beside OP_DOT / OP_L2 / OP_L1 / OP_LINF

// compute() (distances.rs:42-68) after the f32 chain, and similarity_value (distances.rs:122-128): K9's, word for word
template <int OP>
__device__ __forceinline__ float finish_raw(int metric, float acc, const float *q, const float *x, uint32_t d) {
  float raw = acc;
  if (metric == M_NIP) raw = -acc;
  else if (metric == M_L2) raw = finite_f32(acc) ? __builtin_sqrtf(acc) : acc;
  if (!finite_f32(raw)) raw = recover_overflow(metric, q, x, d);
  return raw;
}
__device__ __forceinline__ float similarity(int metric, float raw) {
  if (metric == M_COS || metric == M_IP) return raw;
  if (metric == M_NIP) return -raw;
  return 1.0f / (1.0f + raw);
}

// One pair, one lane, outside the f32 families (K12; K9 and the pass below run the same steps eight query vectors wide):
// cosine() (distances.rs:160-177) over the two vectors' f64 norms -- fma(q, x, acc) == acc + q*x, a product of two f32 is
// exact in f64; NaN: "metric overflow" --
__device__ __forceinline__ float pair_cosine_raw(const float *q, const float *x, uint32_t d, double qn, double xn) {
  double dot = 0.0;
  for (uint32_t e = 0; e < d; ++e) dot = __builtin_fma((double)q[e], (double)x[e], dot);
  if (qn == 0.0 || xn == 0.0) return 0.0f;
  const double sim = dot / (qn * xn);
  return isfinite(sim) ? (float)fmin(fmax(sim, -1.0), 1.0) : __builtin_nanf("");
}
// and hamming() / jaccard() (distances.rs:319-347) over truthiness: integer counts, exact for any d
__device__ __forceinline__ float pair_count_raw(int metric, const float *q, const float *x, uint32_t d) {
  uint32_t ham = 0, inter = 0, uni = 0;
  for (uint32_t e = 0; e < d; ++e) {
    const bool ql = q[e] != 0.0f, xr = x[e] != 0.0f;
    ham += ql != xr;
    inter += ql && xr;
    uni += ql || xr;
  }
  if (metric == M_HAM) return (float)ham;
  return uni == 0 ? 0.0f : 1.0f - (float)inter / (float)uni;
}

// A wave's view of the slab and of its LDS tile: wave-uniform but for the lane's own place in the staging walk.
struct MaxSimTileWalk {
  const float *X;       // the slab, `stride` floats a row
  size_t stride;
  const double *tnorm;  // cosine: per row of X
  float *tile;          // [tt][ld]
  uint32_t d, ttl, ld;
  int metric;
  uint32_t lane;
};

// The maxima over a document's T > 0 rows (first row t0) for this lane's eight query vectors qk[0..8) -- qnorm[qi[k]] their
// norms (cosine) --, reduced over the tt lanes of the lane's query group: best[k] and, for a failed pair anywhere in the
// group, bad[k].  `stage`: the tile does not hold the document yet (a document of one tile stays staged for later passes).
// `qlive`: the lane's group exists (the others compute and drop).
template <int OP, int ORDER>
__device__ __forceinline__ void maxsim_pass(const MaxSimTileWalk &w, uint32_t t0, uint32_t T, bool stage, bool qlive,
                                            const float *const (&qk)[kQB], const double *qnorm, const uint32_t (&qi)[kQB],
                                            float (&best)[kQB], bool (&bad)[kQB]) {
  const uint32_t lane = w.lane, ttl = w.ttl, tt = 1u << ttl, ld = w.ld;
  float *tile = w.tile;
  const uint32_t tok = lane & (tt - 1);
  const int metric = w.metric;
  const uint32_t d = w.d, cfull = d / 8;
  // the staging walk: 16-byte unit u of a tile is (row u / rs4, column u % rs4); a lane takes units lane, lane + 64, ...
  const uint32_t rs4 = (uint32_t)w.stride / 4, ld4 = ld / 4;
  const uint32_t row_first = lane / rs4, col_first = lane % rs4, row_step = kWave / rs4, col_step = kWave % rs4;
#pragma unroll
  for (int k = 0; k < kQB; ++k) {
    best[k] = -__builtin_inff();
    bad[k] = false;
  }
  for (uint32_t j0 = 0; j0 < T; j0 += tt) {
    const uint32_t cnt = T - j0 < tt ? T - j0 : tt;
    if (stage || T > tt) {
      wave_lds_fence();  // the readers of the tile's previous rows are done
      const f32x4 *src = reinterpret_cast<const f32x4 *>(w.X + (size_t)(t0 + j0) * w.stride);
      const uint32_t units = cnt * rs4;
      uint32_t row = row_first, col = col_first;
      for (uint32_t u = lane; u < units; u += kWave) {
        reinterpret_cast<f32x4 *>(tile)[row * ld4 + col] = src[u];
        row += row_step;
        col += col_step;
        if (col >= rs4) {
          col -= rs4;
          ++row;
        }
      }
      wave_lds_fence();
    }
    const bool live = tok < cnt && qlive;  // (the others compute row 0 of the tile and drop it)
    const float *x = tile + (size_t)(tok < cnt ? tok : 0) * ld;
    float raw[kQB];
    if (OP == MS_COS) {
      // distances.rs:160-185 cosine(): fma(q, t, acc) == acc + q*t (a product of two f32 is exact in f64)
      double dot[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) dot[k] = 0.0;
      for (uint32_t e = 0; e < d; ++e) {
        const double xv = (double)x[e];
#pragma unroll
        for (int k = 0; k < kQB; ++k) dot[k] = __builtin_fma((double)qk[k][e], xv, dot[k]);
      }
      const double rn = w.tnorm[t0 + j0 + (tok < cnt ? tok : 0)];
#pragma unroll
      for (int k = 0; k < kQB; ++k) {
        const double ln = qnorm[qi[k]];
        raw[k] = 0.0f;
        if (!(ln == 0.0 || rn == 0.0)) {
          const double sim = dot[k] / (ln * rn);
          raw[k] = isfinite(sim) ? (float)fmin(fmax(sim, -1.0), 1.0) : __builtin_nanf("");
        }
      }
    } else {
      float acc[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) acc[k] = 0.0f;
      for (uint32_t c = 0; c < cfull; ++c) {
        const f32x4 xa = *reinterpret_cast<const f32x4 *>(x + c * 8);
        const f32x4 xb = *reinterpret_cast<const f32x4 *>(x + c * 8 + 4);
#pragma unroll
        for (int k = 0; k < kQB; ++k) {
          const f32x4 qa = *reinterpret_cast<const f32x4 *>(qk[k] + c * 8);
          const f32x4 qb = *reinterpret_cast<const f32x4 *>(qk[k] + c * 8 + 4);
          const float l[8] = {elem<OP>(0, qa.x, xa.x), elem<OP>(0, qa.y, xa.y), elem<OP>(0, qa.z, xa.z),
                              elem<OP>(0, qa.w, xa.w), elem<OP>(0, qb.x, xb.x), elem<OP>(0, qb.y, xb.y),
                              elem<OP>(0, qb.z, xb.z), elem<OP>(0, qb.w, xb.w)};
          acc[k] = comb<OP>(0, acc[k], chunk_sum1<OP, ORDER>(l));
        }
      }
      for (uint32_t e = cfull * 8; e < d; ++e) {  // the scalar tail, one element at a time (never the row's pad)
        const float xe = x[e];
#pragma unroll
        for (int k = 0; k < kQB; ++k) acc[k] = comb<OP>(0, acc[k], elem<OP>(0, qk[k][e], xe));
      }
#pragma unroll
      for (int k = 0; k < kQB; ++k) raw[k] = finish_raw<OP>(metric, acc[k], qk[k], x, d);
    }
#pragma unroll
    for (int k = 0; k < kQB; ++k) {
      if (!live) continue;
      if (raw[k] != raw[k]) bad[k] = true;
      else best[k] = fmaxf(best[k], similarity(metric, raw[k]));
    }
  }
  // The maximum over the document's vectors as a tree over the tt lanes of a query group (K9 says why a tree may
  // stand for the reference's fold in vector order), a failed pair anywhere in the group as a flag.
#pragma unroll
  for (int k = 0; k < kQB; ++k) {
    float b = best[k];
    int f = bad[k] ? 1 : 0;
    for (uint32_t o = tt >> 1; o > 0; o >>= 1) {
      b = fmaxf(b, __shfl_xor(b, (int)o, kWave));
      f |= __shfl_xor(f, (int)o, kWave);
    }
    best[k] = b;
    bad[k] = f != 0;
  }
}

}  // namespace

}  // namespace dev
}  // namespace vt

// vt_maxsim_pair.cuh -- what is MaxSim's own around the pair arithmetic of vt_pair.cuh: the three steps K9 (vt_maxsim.hip),
// K9r (vt_maxsim_resident.hip) and K9rb (vt_maxsim_batch.hip) share, and one wave's pass over one document of a resident
// store for the eight query vectors of each of its lanes (K9r, K9rb).  In the pass a lane is (row of the tile, group of
// eight query vectors); the document's rows come through the wave's LDS tile, `tt` at a time, and every (query vector,
// document vector) pair is one lane's own chain.  K9r and K9rb differ only in where a lane's eight query vectors come
// from and in what they do with the maxima.
#pragma once
#include "vt_pair.cuh"

namespace vt {
namespace dev {

namespace {

constexpr size_t kResidentLds = 128 * 1024;  // LDS of a block: the query panel and four tiles

// The block's query panel into LDS: n4 16-byte units from Q, then the barrier (K9r, K9rb; K9 says why it keeps its own).
__device__ __forceinline__ void stage_query_panel(float *qs, const float *Q, uint32_t n4) {
  const f32x4 *src = reinterpret_cast<const f32x4 *>(Q);
  for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4 *>(qs)[i] = src[i];
  __syncthreads();
}

// One step of the sum over query vectors -- sequential, in query order -- with the reference's error at the first query
// vector that has one: `best` is the vector's maximum over the document, `bad` a failed pair among them (wave-uniform).
__device__ __forceinline__ void add_query_max(float best, bool bad, float &tot, int &st) {
  if (st) return;
  if (bad) {
    st = kErrOverflow;
    return;
  }
  tot += best;
  if (!finite_f32(tot)) st = kErrScoreOverflow;
}

// A finished document, by one lane: key and payload {row, score}, or kEmptyKey and (row << 8 | status) into *first_error
// (atomicMin: the earliest document wins).
__device__ __forceinline__ void write_document(uint64_t *key, Payload *pay, unsigned long long *first_error, uint32_t row,
                                               const uint32_t *id_rank, float tot, int st) {
  if (st) {
    *key = kEmptyKey;
    atomicMin(first_error, ((unsigned long long)row << 8) | (unsigned)st);
  } else {
    *key = ((uint64_t)~orderable(tot) << 32) | *id_rank;  // descending score, then id
    Payload p;
    p.row = row;
    p.raw = tot;
    *pay = p;
  }
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
  const uint32_t d = w.d;
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
    if constexpr (OP == PAIR_COS) {
      double dot[kQB];
      cosine_dots(qk, x, d, dot);
      const double rn = w.tnorm[t0 + j0 + (tok < cnt ? tok : 0)];
#pragma unroll
      for (int k = 0; k < kQB; ++k) raw[k] = cosine_raw(dot[k], qnorm[qi[k]], rn);
    } else {
      f32_raws<OP, ORDER, kQB, false, false>(metric, qk, x, d, raw);
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

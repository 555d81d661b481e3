// vt_rowscore.cuh -- one f32 row scored against the query with K1's arithmetic by one wave, for the kernels that need the
// exact key of a handful of rows (vt_sketch.hip, sketch_refine_kernel; vt_sketch_nibble.cuh, the 4-bit pass's best rows):
// lane l holds the floats [256 s + 4 l, + 4) of segment s, a lane pair an 8-float chunk; elem4 / chunk_sum of vt_scan.cuh
// give the chunk's sum in the index's reduce order, the sums go to an LDS row of ss = ld / 8 + 12 floats (K1's panel row:
// the sums, then the eight products of the tail chunk, which the reference adds one by one), and one lane walks the row --
// the reference's sequential chain, then the scalar tail.  The value and its rank are formed as scan_topk_kernel forms them.
#pragma once
#include "vt_scan.cuh"

namespace vt {
namespace dev {

// The lane's four products at column `col` of the row (a multiple of 4; at or past ld: nothing is written) into Srow.
// Called by whole waves: chunk_sum reads the neighbour lane.
template <int ORDER>
__device__ __forceinline__ void row_chunk(float *Srow, const f32x4 qv, const f32x4 xv, uint32_t col, uint32_t ld, uint32_t cfull,
                                          uint32_t tail_base, int order, int odd) {
  const f32x4 pr = elem4<OP_DOT>(OP_DOT, qv, xv);
  const float sum = chunk_sum<OP_DOT, ORDER>(OP_DOT, order, pr.x, pr.y, pr.z, pr.w, odd);
  const uint32_t ch = col >> 3;
  if (col < ld) {
    if (ch < cfull) {
      if (!odd) Srow[ch] = sum;
    } else if (ch == cfull) {  // the tail chunk: the reference adds these products one by one
      *reinterpret_cast<f32x4 *>(Srow + tail_base + odd * 4) = pr;
    }
  }
}

// One lane down the row's chunk sums in order, then the `tail` products behind them.
__device__ __forceinline__ float row_chain(const float *Sr, uint32_t cfull, uint32_t tail, uint32_t tail_base) {
  float acc = 0.0f;
  uint32_t c = 0;
  for (; c + 4 <= cfull; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(Sr + c);
    acc = acc + v.x;
    acc = acc + v.y;
    acc = acc + v.z;
    acc = acc + v.w;
  }
  for (; c < cfull; ++c) acc = acc + Sr[c];
  for (uint32_t j = 0; j < tail; ++j) acc = acc + Sr[tail_base + j];
  return acc;
}

// The orderable rank word of a dot-family value (distances.rs:113-119 rank_value, flat.rs:34-40 ordering); false when the
// value or its rank is not finite (K1 recovers such a row in f64: its caller here only does without the row).
__device__ __forceinline__ bool row_rank_word(int metric, float acc, uint32_t *word) {
  const float raw = metric == M_NIP ? -acc : acc;
  float rank = raw;
  if (metric == M_COS) rank = 1.0f - raw;
  else if (metric == M_IP) rank = -raw;
  *word = orderable(rank);
  return finite_f32(raw) && finite_f32(rank);
}

}  // namespace dev
}  // namespace vt

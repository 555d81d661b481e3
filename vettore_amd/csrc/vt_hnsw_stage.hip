// vt_hnsw_stage.hip -- K15: the two scoring kernels behind an HNSW collection's staged searches (quantized_search,
// funnel_search, hybrid_search: collection.ex:232-348) (gfx950).  Both read the slab of the HNSW index where it lies --
// f32 rows `stride` = round_up(d, 4) floats apart, dead rows between live ones, no derived column -- and both write one
// key and one payload per scanned position in the key-column convention (vt_device.h): key = orderable(rank) << 32 |
// id_rank[row], Payload{row, raw}, kEmptyKey for a position that does not take part.  K3 selects behind them.
//
// K15b, hnsw_stage_bits_kernel: packed_hamming (distances.rs:426-437) of compress_sign_bits(row) against the query's
// sign bits, for every slab row.  One wave per row.  A lane loads 16 bytes: floats 4 * lane .. 4 * lane + 3 of a 256-float
// chunk, and __ballot(x >= 0.0f) over component j of all lanes is a 64-bit word of the row's sign bits -- not the
// reference's word (that one holds 64 consecutive elements) but the same bits in another order, and a Hamming distance
// does not care as long as the query's bits come in that order too: hnsw_stage_qwords (vt_device.h) lays them out, once
// per query, with every bit at or past d clear; a lane's elements at or past d are kept out of the ballot.  The XOR, the
// population count and the sum are wave-uniform; lane 0 stores.  The kernel reads 32 times the bytes a bit column would
// hold: deliberate (no column to keep through growth, upsert and compaction).
//
// K15p, hnsw_stage_score_kernel: vector_top_k's value (search.rs:38-73) on the first p <= d coordinates -- compute(query,
// row) in the f32 families, the f64 cosine with both norms over the prefix -- of every slab row or of the rows a device
// list names (position i belongs to list[i]).  The arithmetic is vt_pair.cuh's, one lane walking one pair, the query
// on the left.  One block is one wave; it takes groups of `tt` positions: the first round_up(p, 4) floats of their
// rows are staged into an LDS tile with coalesced 16-byte loads, the query's prefix sits in LDS beside it, and lane r walks
// row r of the tile.  Prefixes longer than kHnswLdsDim floats are walked where they lie, 64 positions a group, as K11
// does.  A raw value that is NaN ("metric overflow") raises *status to kErrOverflow and leaves kEmptyKey.
#include "vt_pair.cuh"

namespace vt {
namespace dev {

namespace {

constexpr uint32_t kStageMaxBlocks = 2048;

__global__ __launch_bounds__(kWavesPerBlock *kWave) void hnsw_stage_bits_kernel(const HnswStageBitsArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t nwaves = gridDim.x * kWavesPerBlock;
  const uint32_t chunks = (a.d + 255) / 256;
  for (uint32_t row = wave; row < a.rows; row += nwaves) {  // (wave-uniform)
    const uint32_t rk = a.id_rank[row];
    if (rk == kHnswNoRow) {
      if (lane == 0) {
        a.keys[row] = kEmptyKey;
        a.pay[row] = Payload{row, 0.0f};
      }
      continue;
    }
    const float *x = a.X + (size_t)row * a.stride;
    uint32_t count = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
      const uint32_t e = c * 256 + 4 * lane;  // (a multiple of 4: below the stride the whole load is)
      f32x4 v = {-1.0f, -1.0f, -1.0f, -1.0f};
      if (e < a.d) v = *reinterpret_cast<const f32x4 *>(x + e);
      const uint64_t *qw = a.qwords + 4 * (size_t)c;
      count += (uint32_t)__popcll(__ballot(e + 0 < a.d && v.x >= 0.0f) ^ qw[0]);
      count += (uint32_t)__popcll(__ballot(e + 1 < a.d && v.y >= 0.0f) ^ qw[1]);
      count += (uint32_t)__popcll(__ballot(e + 2 < a.d && v.z >= 0.0f) ^ qw[2]);
      count += (uint32_t)__popcll(__ballot(e + 3 < a.d && v.w >= 0.0f) ^ qw[3]);
    }
    if (lane == 0) {
      const float raw = (float)count;
      a.keys[row] = ((uint64_t)orderable(raw) << 32) | rk;
      a.pay[row] = Payload{row, raw};
    }
  }
}

__device__ __forceinline__ float stage_rank_of(int metric, float raw) {  // distances.rs:113-119 rank_value
  if (metric == M_COS) return 1.0f - raw;
  if (metric == M_IP) return -raw;
  return raw;
}

// LDS: [64] the group's rows, [round_up(p, 4)] the query's prefix, [tt][ld] the tile (STAGED); nothing otherwise
template <int OP, int ORDER, bool STAGED>
__global__ __launch_bounds__(kWave) void hnsw_stage_score_kernel(const HnswStageScoreArgs a) {
  extern __shared__ __align__(16) float lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t p = a.p;
  uint32_t *grows = reinterpret_cast<uint32_t *>(lds);
  float *qs = lds + kWave;
  float *tile = qs + round_up(p, 4);
  if (STAGED) {
    for (uint32_t i = lane; i < p; i += kWave) qs[i] = a.q[i];
    wave_lds_fence();
  }
  const float *q = STAGED ? qs : a.q;
  const uint32_t step = STAGED ? a.tt : (uint32_t)kWave;
  const uint32_t ngroups = (a.n + step - 1) / step;
  for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {  // (wave-uniform)
    const uint32_t g0 = g * step;
    const uint32_t cnt = a.n - g0 < step ? a.n - g0 : step;
    // the row of position g0 + lane, and whether it takes part: a row of the slab that is live
    uint32_t row = kHnswNoRow, rk = kHnswNoRow;
    if (lane < cnt) {
      row = a.list ? a.list[g0 + lane] : g0 + lane;
      if (row < a.rows) rk = a.id_rank[row];
    }
    const bool live = rk != kHnswNoRow;
    if (STAGED) {
      wave_lds_fence();  // the readers of the previous group's rows are done
      grows[lane] = live ? row : kHnswNoRow;
      wave_lds_fence();
      const uint32_t rs4 = round_up(p, 4) / 4, ld4 = a.ld / 4;
      const uint32_t units = cnt * rs4;
      for (uint32_t u = lane; u < units; u += kWave) {
        const uint32_t r = u / rs4, c = u - r * rs4;
        const uint32_t src_row = grows[r];
        if (src_row == kHnswNoRow) continue;
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.X + (size_t)src_row * a.stride);
        reinterpret_cast<f32x4 *>(tile)[r * ld4 + c] = src[c];
      }
      wave_lds_fence();
    }
    float raw = 0.0f;
    if (live) {  // (lane < cnt)
      const float *x = STAGED ? tile + (size_t)lane * a.ld : a.X + (size_t)row * a.stride;
      if constexpr (OP == PAIR_COS) {
        const float *const v[2] = {q, x};
        double dot[2];
        cosine_dots<2>(v, x, p, dot);  // q.x and x.x, each sequentially in f64
        raw = cosine_raw(dot[0], sqrt(a.qq), sqrt(dot[1]));
      } else {
        const float *const v[1] = {q};
        float r1[1];
        f32_raws<OP, ORDER, 1, false, false>(a.metric, v, x, p, r1);  // left = query, right = stored row
        raw = r1[0];
      }
    }
    const bool ok = live && raw == raw;
    if (live && !ok) atomicMax(a.status, kErrOverflow);
    if (lane < cnt) {
      a.keys[g0 + lane] = ok ? (((uint64_t)orderable(stage_rank_of(a.metric, raw)) << 32) | rk) : kEmptyKey;
      a.pay[g0 + lane] = Payload{row, raw};
    }
  }
}

// tile rows and the floats between them for a prefix of p floats: a pitch whose count of 16-byte slots is odd, so that
// the lanes' 16-byte reads of one column spread over the banks; as many rows (a power of two, at most 64) as 64 KiB hold
// beside the query and the row list
void stage_tile_plan(uint32_t p, uint32_t *tt, uint32_t *ld) {
  *tt = 0;
  *ld = 0;
  if (p > kHnswLdsDim) return;
  const uint32_t rp = round_up(p, 4);
  const uint32_t l = (rp / 4) % 2 ? rp : rp + 4;
  const size_t room = 64 * 1024 - (size_t)(kWave + rp) * sizeof(float);
  uint32_t t = 64;
  while (t > 1 && (size_t)t * l * sizeof(float) > room) t >>= 1;
  *tt = t;
  *ld = l;
}

template <int OP, int ORDER>
hipError_t launch_score_t(HnswStageScoreArgs a, hipStream_t s) {
  stage_tile_plan(a.p, &a.tt, &a.ld);
  const bool staged = a.tt != 0;
  const uint32_t step = staged ? a.tt : (uint32_t)kWave;
  const uint32_t ngroups = (a.n + step - 1) / step;
  const uint32_t blocks = ngroups < 2 * kStageMaxBlocks ? ngroups : 2 * kStageMaxBlocks;
  if (staged) {
    const size_t lds = (size_t)(kWave + round_up(a.p, 4) + (size_t)a.tt * a.ld) * sizeof(float);
    hipLaunchKernelGGL((hnsw_stage_score_kernel<OP, ORDER, true>), dim3(blocks), dim3(kWave), lds, s, a);
  } else {
    hipLaunchKernelGGL((hnsw_stage_score_kernel<OP, ORDER, false>), dim3(blocks), dim3(kWave), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

void hnsw_stage_qwords(const float *q, uint32_t d, uint64_t *out) {
  const size_t words = hnsw_stage_qword_count(d);
  for (size_t w = 0; w < words; ++w) out[w] = 0;
  for (uint32_t e = 0; e < d; ++e)
    if (q[e] >= 0.0f) out[4 * (size_t)(e / 256) + e % 4] |= 1ull << (e % 256 / 4);
}

hipError_t launch_hnsw_stage_bits(const HnswStageBitsArgs &a, hipStream_t s) {
  if (a.rows == 0) return hipSuccess;
  if (a.d == 0 || a.stride % 4 || a.stride < a.d || a.rows == kHnswNoRow) return hipErrorInvalidValue;
  const uint32_t want = (a.rows + kWavesPerBlock - 1) / kWavesPerBlock;
  const uint32_t blocks = want < dev::kStageMaxBlocks ? want : dev::kStageMaxBlocks;
  hipLaunchKernelGGL(dev::hnsw_stage_bits_kernel, dim3(blocks), dim3(kWavesPerBlock * dev::kWave), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_hnsw_stage_score(const HnswStageScoreArgs &a, hipStream_t s) {
  using namespace dev;
  if (a.n == 0) return hipSuccess;
  if (a.p == 0 || a.p > a.d || a.stride % 4 || a.stride < a.d || a.rows == kHnswNoRow || (!a.list && a.n > a.rows))
    return hipErrorInvalidValue;
  if (a.metric != M_COS && a.metric != M_IP && a.metric != M_L2) return hipErrorInvalidValue;  // (the index's three metrics)
  return dispatch_pair<1u << OP_DOT | 1u << OP_L2 | kPairCos>(
      a.metric, a.order, [&](auto op, auto order) { return launch_score_t<op(), order()>(a, s); });
}

}  // namespace vt

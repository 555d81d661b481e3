// vt_mmr.hip -- K12: the MMR step kernel (gfx950).
//
// Replaces do_mmr / score_mmr_candidates / maximum_redundancy (lib/vettore_distance.ex:416-487) and the NIF call per
// pair behind pair_similarity (:489-519).  Protocol, layout and phases: MmrArgs in vt_device.h.  What makes one launch
// per round enough: the redundancy of a candidate is a maximum over the chosen, and a maximum can be carried -- round t
// scores every live candidate against the ONE row chosen in round t - 1 and folds it into the candidate's f64 state.
// A pair is computed in the round in which the reference first computes it, so its "metric overflow" fails the call in
// the same round; a round that never runs computes nothing.
//
// Arithmetic: one lane computes one (candidate, winner) pair from start to finish, candidate on the left: vt_pair.cuh's
// three families, one pair wide, cosine over the two rows' f64 norms, each computed once, in launch 0; then
// pair_similarity's f64 value and the f64 score.  The choice is a reduction under the key (largest score, smallest
// candidate): Enum.max_by keeps the first maximum, and the remaining candidates keep their list order.
#include "vt_pair.cuh"

namespace vt {
namespace dev {

namespace {

constexpr int kMmrThreads = 256;
constexpr uint32_t kMmrHeadBytes = 80;  // the waves' reduction slots (4 x 16) and the round's {winner, failed}; a multiple of 16

// compute(metric, q, x) (distances.rs:42-68; cosine over the norms qn / xn): vt_pair.cuh's, one pair wide.
// NaN: "metric overflow".
template <int OP, int ORDER>
__device__ __forceinline__ float pair_raw(int metric, const float *q, const float *x, uint32_t d, double qn, double xn) {
  const float *const qv[1] = {q};
  float raw[1];
  if constexpr (OP == PAIR_COS) {
    double dot[1];
    cosine_dots(qv, x, d, dot);
    raw[0] = cosine_raw(dot[0], qn, xn);
  } else if constexpr (OP == PAIR_COUNT) {
    count_raws(metric, qv, x, d, raw);
  } else {
    f32_raws<OP, ORDER, 1, false, false>(metric, qv, x, d, raw);
  }
  return raw[0];
}

// pair_similarity (vettore_distance.ex:489-519): the f32 raw value as a double, then the metric's f64 step
__device__ __forceinline__ double mmr_similarity(int metric, float raw) {
  if (metric == M_COS || metric == M_IP) return (double)raw;
  if (metric == M_NIP) return -(double)raw;
  return 1.0 / (1.0 + (double)raw);
}

// (largest score, smallest candidate) and the smallest failed candidate
__device__ __forceinline__ void mmr_merge(MmrPartial &a, double score, uint32_t best, uint32_t failed) {
  if (best != kMmrNone && (a.best == kMmrNone || score > a.score || (score == a.score && best < a.best))) {
    a.score = score;
    a.best = best;
  }
  a.failed = failed < a.failed ? failed : a.failed;
}
__device__ __forceinline__ MmrPartial mmr_wave_reduce(MmrPartial v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double s = __shfl_xor(v.score, o, kWave);
    const uint32_t b = (uint32_t)__shfl_xor((int)v.best, o, kWave);
    const uint32_t f = (uint32_t)__shfl_xor((int)v.failed, o, kWave);
    mmr_merge(v, s, b, f);
  }
  return v;
}

template <int OP, int ORDER, bool STAGED>
__global__ __launch_bounds__(kMmrThreads) void mmr_step_kernel(const MmrArgs a, const uint32_t t) {
  extern __shared__ __align__(16) unsigned char mmr_lds[];
  MmrPartial *wred = reinterpret_cast<MmrPartial *>(mmr_lds);          // [4]
  uint32_t *head = reinterpret_cast<uint32_t *>(mmr_lds + 64);         // {winner, failed}
  float *sel = reinterpret_cast<float *>(mmr_lds + kMmrHeadBytes);     // the winner's row (STAGED)
  const uint32_t p = blockIdx.y, b = blockIdx.x, B = gridDim.x, tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const MmrProblem pr = a.prob[p];
  if (t == 0 && b == 0 && tid == 0) {
    a.count[p] = 0;
    a.status[p] = 0;
  }
  if (t > pr.kk) return;  // finished (or failed) in an earlier launch
  MmrPartial *cur = a.partial + ((size_t)(t & 1) * gridDim.y + p) * B;

  // ---- phase A: the choice of round t - 1
  uint32_t winner = kMmrNone;
  if (t >= 1) {
    const MmrPartial *prev = a.partial + ((size_t)((t - 1) & 1) * gridDim.y + p) * B;
    if (wib == 0) {
      MmrPartial v;
      v.score = 0.0;
      v.best = v.failed = kMmrNone;
      if ((uint32_t)lane < B) v = prev[lane];
      v = mmr_wave_reduce(v);
      if (lane == 0) {
        head[0] = v.best;
        head[1] = v.failed;
      }
    }
    __syncthreads();
    winner = head[0];
    const uint32_t failed = head[1];
    if (failed != kMmrNone) {  // (block-uniform) "metric overflow" in round t - 1, or handed on from an earlier one
      if (tid == 0) {
        MmrPartial v;
        v.score = 0.0;
        v.best = kMmrNone;
        v.failed = failed;
        if (t < pr.kk) cur[b] = v;
        if (b == 0) a.status[p] = kErrOverflow;
      }
      return;
    }
    if (winner >= pr.n) return;  // (cannot be: a round that ran left a best or a failed candidate; the host sees a short count)
    if (b == 0 && tid == 0) {
      a.order_out[pr.off + t - 1] = winner;
      a.count[p] = t;
    }
  }
  if (t >= pr.kk) return;

  // ---- phase B: round t's scores
  const float *x = nullptr;
  double xn = 0.0;
  if (t >= 1) {
    const float *wrow = a.X + (size_t)a.rows[pr.off + winner] * a.stride;
    if (OP == PAIR_COS) xn = a.norm[pr.off + winner];
    x = wrow;
    if (STAGED) {
      const uint32_t d4 = (a.d + 3) / 4;  // (a row's stride is a multiple of 4 floats: the pad is read, never used)
      for (uint32_t j = tid; j < d4; j += kMmrThreads) reinterpret_cast<f32x4 *>(sel)[j] = reinterpret_cast<const f32x4 *>(wrow)[j];
      __syncthreads();
      x = sel;
    }
  }
  MmrPartial mine;
  mine.score = 0.0;
  mine.best = mine.failed = kMmrNone;
  const uint32_t br = a.block_rows;
  for (uint64_t base = (uint64_t)b * br; base < pr.n; base += (uint64_t)B * br) {
    const uint32_t i = (uint32_t)base + tid;
    if (tid >= br || i >= pr.n) continue;
    const size_t gi = (size_t)pr.off + i;
    const float *q = a.X + (size_t)a.rows[gi] * a.stride;
    double red = 0.0;  // maximum_redundancy with nothing chosen
    if (t == 0) {
      a.live[gi] = 1;
      if (OP == PAIR_COS) {
        double acc = 0.0;
        for (uint32_t e = 0; e < a.d; ++e) acc = __builtin_fma((double)q[e], (double)q[e], acc);
        a.norm[gi] = sqrt(acc);
      }
    } else {
      if (i == winner) {
        a.live[gi] = 0;
        continue;
      }
      if (!a.live[gi]) continue;
      const float raw = pair_raw<OP, ORDER>(a.metric, q, x, a.d, OP == PAIR_COS ? a.norm[gi] : 0.0, xn);
      if (raw != raw) {
        mine.failed = i < mine.failed ? i : mine.failed;
        continue;
      }
      const double sim = mmr_similarity(a.metric, raw);
      red = sim;  // maximum_similarity(nil, similarity): the first one replaces the state, it is not compared with 0.0
      if (t >= 2) {
        const double old = a.red[gi];
        red = sim > old ? sim : old;
      }
      a.red[gi] = red;
    }
    // Two products and a subtraction, each rounded: `#pragma clang fp contract(off)` (vt_common.cuh) covers this file, so
    // no FMA is formed here whatever the command line says -- a fused score selects other rows (tests/test_mmr_ref.py).
    const double score = pr.alpha * a.rel[gi] - (1.0 - pr.alpha) * red;
    mmr_merge(mine, score, i, kMmrNone);
  }
  mine = mmr_wave_reduce(mine);
  if (lane == 0) wred[wib] = mine;
  __syncthreads();
  if (tid == 0) {
    MmrPartial v = wred[0];
    for (int w = 1; w < kMmrThreads / kWave; ++w) mmr_merge(v, wred[w].score, wred[w].best, wred[w].failed);
    cur[b] = v;
  }
}

template <int OP, int ORDER>
hipError_t launch_t(const MmrArgs &a, uint32_t t, uint32_t blocks, uint32_t nprob, hipStream_t s) {
  const size_t lds = mmr_lds_bytes(a.d, a.lds_dim);
  if (a.d <= a.lds_dim)
    hipLaunchKernelGGL((mmr_step_kernel<OP, ORDER, true>), dim3(blocks, nprob), dim3(kMmrThreads), lds, s, a, t);
  else
    hipLaunchKernelGGL((mmr_step_kernel<OP, ORDER, false>), dim3(blocks, nprob), dim3(kMmrThreads), lds, s, a, t);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

size_t mmr_lds_bytes(uint32_t d, uint32_t lds_dim) {
  return dev::kMmrHeadBytes + (d <= lds_dim ? (size_t)dev::round_up(d, 4) * sizeof(float) : 0);
}

hipError_t launch_mmr_step(const MmrArgs &a, uint32_t t, uint32_t blocks, uint32_t nprob, hipStream_t s) {
  using namespace dev;
  if (nprob == 0) return hipSuccess;
  if (blocks == 0 || blocks > kMmrMaxBlocks || nprob > 65535u || a.block_rows == 0 || a.block_rows > kMmrBlockRows ||
      a.lds_dim > kMmrLdsDim || (a.stride & 3u) != 0)
    return hipErrorInvalidValue;
  return dispatch_pair<kPairF32 | kPairCos | kPairCount>(
      a.metric, a.order, [&](auto op, auto order) { return launch_t<op(), order()>(a, t, blocks, nprob, s); });
}

}  // namespace vt

// vt_maxsim.hip -- K9: MaxSim / ColBERT scoring of multi-vector documents (gfx950).
//
// Replaces score_validated (native/vettore/src/multi_vector.rs:65-88) under multi_vector_top_k / _score.
// Layout: MaxSimArgs in vt_device.h.  Arithmetic: vt_pair.cuh -- one lane computes one (query vector, document
// vector) pair from start to finish, so the reference's order needs no cross-lane exchange; cosine runs over the norms
// of launch_maxsim_norms (each vector's once per call).  A lane walks eight query vectors at once: a document vector's
// chunk is loaded once for eight chains.  A lane reads its document vector where it lies in global memory, and a row
// there starts at a multiple of `stride` >= d floats, which need not be 16 bytes: the row's chunk is eight scalar loads.
#include "vt_maxsim_pair.cuh"  // the arithmetic (vt_pair.cuh) and the steps shared with K9r and K9rb

namespace vt {
namespace dev {

namespace {

constexpr size_t kPanelLds = 64 * 1024;      // LDS for the query panel (more only when one vector needs it)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

template <int OP, int ORDER>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void maxsim_kernel(const MaxSimArgs a) {
  extern __shared__ __align__(16) float qs[];  // [panel_qn][q_stride]
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t qn = a.panel_qn, qst = a.q_stride;
  {  // (stage_query_panel's lines, kept here: through the call this kernel's f64 dot loop came out with one load in flight)
    const f32x4 *src = reinterpret_cast<const f32x4 *>(a.Q + (size_t)a.panel_q0 * qst);
    const uint32_t n4 = qn * qst / 4;
    for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4 *>(qs)[i] = src[i];
  }
  __syncthreads();
  const int metric = a.metric;
  const uint32_t d = a.d;
  const bool first_panel = a.panel_q0 == 0, last_panel = a.panel_q0 + qn >= a.nq;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;

  for (uint32_t i = blockIdx.x * kWavesPerBlock + wib; i < a.ndoc; i += total_waves) {
    const uint32_t t0 = a.nq ? a.doc_off[i] : 0u;
    const uint32_t T = !a.nq ? 0u : a.doc_cnt ? a.doc_cnt[i] : a.doc_off[i + 1] - t0;  // (a document without vectors scores 0.0)
    float tot = first_panel ? 0.0f : a.total[i];
    int st = first_panel ? 0 : a.status[i];
    for (uint32_t g = 0; g < qn && T && !st; g += kQB) {
      const float *qk[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) qk[k] = qs + (size_t)(g + k < qn ? g + k : qn - 1) * qst;
      float best[kQB];
      bool bad[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) {
        best[k] = -__builtin_inff();
        bad[k] = false;
      }
      for (uint32_t j = lane; j < T; j += kWave) {
        const float *x = a.X + (size_t)(t0 + j) * a.stride;
        float raw[kQB];
        if constexpr (OP == PAIR_COS) {
          double dot[kQB];
          cosine_dots(qk, x, d, dot);
          const double rn = a.tnorm[t0 + j];
#pragma unroll
          for (int k = 0; k < kQB; ++k) raw[k] = cosine_raw(dot[k], a.qnorm[a.panel_q0 + (g + k < qn ? g + k : qn - 1)], rn);
        } else if constexpr (OP == PAIR_COUNT) {
          count_raws(metric, qk, x, d, raw);
        } else {
          f32_raws<OP, ORDER, kQB, false, true>(metric, qk, x, d, raw);
        }
#pragma unroll
        for (int k = 0; k < kQB; ++k) {
          if (raw[k] != raw[k]) bad[k] = true;
          else best[k] = fmaxf(best[k], similarity(metric, raw[k]));
        }
      }
      // The maximum over the document's vectors as a tree: the reference folds f32::max in vector order
      // (multi_vector.rs:73-81).  No NaN reaches either fold (inputs are finite, a non-finite metric value
      // is an error), and max is exact, so the only freedom is the sign of a zero maximum -- which cannot
      // reach the result: the total starts at +0.0 and x + (-0.0) == x + (+0.0) for every x that is not
      // -0.0, while a sum that starts at +0.0 is never -0.0 in round-to-nearest.
#pragma unroll
      for (int k = 0; k < kQB; ++k) {
        best[k] = wave_max(best[k]);
        bad[k] = __ballot(bad[k]) != 0;
      }
      // the sum over query vectors: sequential, in query order, and the reference's error at the first
      // query vector that has one (every lane holds the same values: the walk is wave-uniform)
#pragma unroll
      for (int k = 0; k < kQB; ++k)
        if (g + k < qn) add_query_max(best[k], bad[k], tot, st);
    }
    if (lane != 0) continue;
    if (!last_panel) {
      a.total[i] = tot;
      a.status[i] = st;
      continue;
    }
    write_document(a.keys + i, a.pay + i, a.first_error, a.row0 + i, a.id_rank + i, tot, st);
  }
}

__global__ void maxsim_norms_kernel(const float *X, size_t stride, uint32_t n, uint32_t d, double *norms) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = X + (size_t)i * stride;
  double acc = 0.0;
  for (uint32_t e = 0; e < d; ++e) acc = __builtin_fma((double)x[e], (double)x[e], acc);
  norms[i] = sqrt(acc);
}

template <int OP, int ORDER>
hipError_t launch_t(const MaxSimArgs &a, uint32_t blocks, hipStream_t s) {
  auto kern = maxsim_kernel<OP, ORDER>;
  const size_t lds = maxsim_lds_bytes(a.panel_qn, a.q_stride);
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

uint32_t maxsim_panel_rows(uint32_t d, uint32_t *q_stride) {
  const uint32_t qst = dev::round_up(d, 8);
  *q_stride = qst;
  const size_t row = (size_t)qst * sizeof(float);
  if (row > dev::kMaxLds) return 0;
  return row > dev::kPanelLds ? 1u : (uint32_t)(dev::kPanelLds / row);
}

size_t maxsim_lds_bytes(uint32_t panel_qn, uint32_t q_stride) {
  return std::max<size_t>((size_t)panel_qn * q_stride * sizeof(float), 16);
}

hipError_t launch_maxsim(const MaxSimArgs &a, uint32_t blocks, hipStream_t s) {
  using namespace dev;
  if (a.nq == 0) return launch_t<PAIR_COUNT, 0>(a, blocks, s);  // (no pair to score: any instance writes the keys)
  return dispatch_pair<kPairF32 | kPairCos | kPairCount>(
      a.metric, a.order, [&](auto op, auto order) { return launch_t<op(), order()>(a, blocks, s); });
}

hipError_t launch_maxsim_norms(const float *X, size_t stride, uint32_t n, uint32_t d, double *norms, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::maxsim_norms_kernel, dim3((n + 255) / 256), dim3(256), 0, s, X, stride, n, d, norms);
  return hipGetLastError();
}

}  // namespace vt

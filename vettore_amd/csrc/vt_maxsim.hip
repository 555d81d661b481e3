// vt_maxsim.hip -- K9: MaxSim / ColBERT scoring of multi-vector documents (gfx950).
//
// Replaces score_validated (native/vettore/src/multi_vector.rs:65-88) under multi_vector_top_k / _score.
// Layout and arithmetic: MaxSimArgs in vt_device.h.  One lane computes one (query vector, document vector)
// pair from start to finish, so the reference's order needs no cross-lane exchange:
//   * eight metrics: per 8-float chunk eight separately rounded products (elem), the chunk folded in the
//     selected lane order (chunk_sum1), `acc += chunk` in chunk order, then the scalar tail and compute()'s
//     finish with the f64 recovery of a non-finite value (recover_overflow) -- K1's arithmetic, one lane wide;
//   * Hamming and Jaccard count in integers (no 4096 trick: any d is exact), as hamming() / jaccard() do;
//   * cosine: f64 q.t sequentially, over the norms of launch_maxsim_norms (each vector's once per call).
// A lane walks eight query vectors at once: a document vector's chunk is loaded once for eight chains.
#include "vt_scan.cuh"

namespace vt {
namespace dev {

namespace {

constexpr int kQB = 8;                        // query vectors per lane pass
constexpr size_t kPanelLds = 64 * 1024;      // LDS for the query panel (more only when one vector needs it)
enum { MS_COS = 6, MS_COUNT = 7 };           // the two families beside OP_DOT / OP_L2 / OP_L1 / OP_LINF

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// compute() (distances.rs:42-68) after the f32 chain: the metric's finish, then the f64 recovery of a
// non-finite value.  NaN = "metric overflow".
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

template <int OP, int ORDER>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void maxsim_kernel(const MaxSimArgs a) {
  extern __shared__ __align__(16) float qs[];  // [panel_qn][q_stride]
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t qn = a.panel_qn, qst = a.q_stride;
  {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(a.Q + (size_t)a.panel_q0 * qst);
    const uint32_t n4 = qn * qst / 4;
    for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) reinterpret_cast<f32x4 *>(qs)[i] = src[i];
  }
  __syncthreads();
  const int metric = a.metric;
  const uint32_t d = a.d, cfull = d / 8;
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
          const double rn = a.tnorm[t0 + j];
#pragma unroll
          for (int k = 0; k < kQB; ++k) {
            const double ln = a.qnorm[a.panel_q0 + (g + k < qn ? g + k : qn - 1)];
            raw[k] = 0.0f;
            if (!(ln == 0.0 || rn == 0.0)) {
              const double sim = dot[k] / (ln * rn);
              raw[k] = isfinite(sim) ? (float)fmin(fmax(sim, -1.0), 1.0) : __builtin_nanf("");
            }
          }
        } else if (OP == MS_COUNT) {
          // distances.rs:319-347 over truthiness: integer counts, exact for any d
          uint32_t ham[kQB], inter[kQB], uni[kQB];
#pragma unroll
          for (int k = 0; k < kQB; ++k) ham[k] = inter[k] = uni[k] = 0;
          for (uint32_t e = 0; e < d; ++e) {
            const bool xr = x[e] != 0.0f;
#pragma unroll
            for (int k = 0; k < kQB; ++k) {
              const bool ql = qk[k][e] != 0.0f;
              ham[k] += ql != xr;
              inter[k] += ql && xr;
              uni[k] += ql || xr;
            }
          }
#pragma unroll
          for (int k = 0; k < kQB; ++k) {
            if (metric == M_HAM) raw[k] = (float)ham[k];
            else raw[k] = uni[k] == 0 ? 0.0f : 1.0f - (float)inter[k] / (float)uni[k];
          }
        } else {
          float acc[kQB];
#pragma unroll
          for (int k = 0; k < kQB; ++k) acc[k] = 0.0f;
          for (uint32_t c = 0; c < cfull; ++c) {
            float xv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = x[c * 8 + e];
#pragma unroll
            for (int k = 0; k < kQB; ++k) {
              const f32x4 qa = *reinterpret_cast<const f32x4 *>(qk[k] + c * 8);
              const f32x4 qb = *reinterpret_cast<const f32x4 *>(qk[k] + c * 8 + 4);
              const float l[8] = {elem<OP>(0, qa.x, xv[0]), elem<OP>(0, qa.y, xv[1]), elem<OP>(0, qa.z, xv[2]),
                                  elem<OP>(0, qa.w, xv[3]), elem<OP>(0, qb.x, xv[4]), elem<OP>(0, qb.y, xv[5]),
                                  elem<OP>(0, qb.z, xv[6]), elem<OP>(0, qb.w, xv[7])};
              acc[k] = comb<OP>(0, acc[k], chunk_sum1<OP, ORDER>(l));
            }
          }
          for (uint32_t e = cfull * 8; e < d; ++e) {  // the scalar tail, one element at a time
            const float xe = x[e];
#pragma unroll
            for (int k = 0; k < kQB; ++k) acc[k] = comb<OP>(0, acc[k], elem<OP>(0, qk[k][e], xe));
          }
#pragma unroll
          for (int k = 0; k < kQB; ++k) raw[k] = finish_raw<OP>(metric, acc[k], qk[k], x, d);
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
      for (int k = 0; k < kQB; ++k) {
        if (st || g + k >= qn) continue;
        if (bad[k]) {
          st = kErrOverflow;
          continue;
        }
        tot += best[k];
        if (!finite_f32(tot)) st = kErrScoreOverflow;
      }
    }
    if (lane != 0) continue;
    if (!last_panel) {
      a.total[i] = tot;
      a.status[i] = st;
      continue;
    }
    if (st) {
      a.keys[i] = kEmptyKey;
      atomicMin(a.first_error, ((unsigned long long)(a.row0 + i) << 8) | (unsigned)st);
    } else {
      a.keys[i] = ((uint64_t)~orderable(tot) << 32) | a.id_rank[i];  // descending score, then id
      Payload p;
      p.row = a.row0 + i;
      p.raw = tot;
      a.pay[i] = p;
    }
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

template <int OP>
hipError_t launch_ordered(const MaxSimArgs &a, uint32_t blocks, hipStream_t s) {
  switch (a.order) {
    case 0: return launch_t<OP, 0>(a, blocks, s);
    case 1: return launch_t<OP, 1>(a, blocks, s);
    case 2: return launch_t<OP, 2>(a, blocks, s);
    default: return launch_t<OP, 3>(a, blocks, s);
  }
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
  if (a.nq == 0) return launch_t<MS_COUNT, 0>(a, blocks, s);  // (no pair to score: any instance writes the keys)
  switch (a.metric) {
    case M_COS: return launch_t<MS_COS, 0>(a, blocks, s);
    case M_HAM:
    case M_JAC: return launch_t<MS_COUNT, 0>(a, blocks, s);
    case M_IP:
    case M_NIP: return launch_ordered<OP_DOT>(a, blocks, s);
    case M_L2:
    case M_L2SQ: return launch_ordered<OP_L2>(a, blocks, s);
    case M_L1: return launch_ordered<OP_L1>(a, blocks, s);
    default: return launch_ordered<OP_LINF>(a, blocks, s);
  }
}

hipError_t launch_maxsim_norms(const float *X, size_t stride, uint32_t n, uint32_t d, double *norms, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::maxsim_norms_kernel, dim3((n + 255) / 256), dim3(256), 0, s, X, stride, n, d, norms);
  return hipGetLastError();
}

}  // namespace vt

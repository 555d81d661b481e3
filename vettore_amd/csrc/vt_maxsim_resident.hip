// vt_maxsim_resident.hip -- K9r: MaxSim over documents that stay in device memory (vt_mv, host/vt_mvstore.h) (gfx950).
//
// K9's arithmetic (vt_pair.cuh: one lane computes one (query vector, document vector) pair from start to finish, so
// the reference's order needs no cross-lane exchange), fed differently.  K9 lets every lane walk its own document
// vector out of global memory, `stride * 4` bytes from its neighbour's: one load instruction touches 64 cache lines.
// Here a wave takes one document of the slot list at a time and brings its token rows into its own LDS tile with
// coalesced 16-byte loads -- the rows of a document are one contiguous run of the slab --, `tt` rows per tile; a lane
// then reads ITS row out of LDS.  The tile's rows are `ld` floats apart with ld / 4 odd, so the 64 lanes' 16-byte reads
// of one column fall into different banks.
// Lane mapping: lane = (token of the tile, group of eight query vectors).  tt is 64, 32 or 16 (the launcher chooses by
// the number of query vectors), so 64 / tt query groups run side by side: a document with 16 tokens and 32 query
// vectors keeps all 64 lanes busy, and its tokens are staged once for all 32.  The maximum over the document's tokens is a
// reduction over the tt lanes of a group; the sum over query vectors stays one sequential wave-uniform f32 chain in
// query order (the groups' maxima are broadcast in that order), with the error of the first query vector that has one.
#include "vt_maxsim_pair.cuh"  // the pass over one document, shared with K9rb (vt_maxsim_batch.hip)

namespace vt {
namespace dev {

namespace {

template <int OP, int ORDER>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void maxsim_resident_kernel(const MaxSimArgs a, const uint32_t ttl,
                                                                               const uint32_t ld) {
  extern __shared__ __align__(16) float lds[];  // [panel_qn][q_stride], then per wave [tt][ld]
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t qn = a.panel_qn, qst = a.q_stride;
  float *qs = lds;
  stage_query_panel(qs, a.Q + (size_t)a.panel_q0 * qst, qn * qst / 4);
  const uint32_t tt = 1u << ttl, groups = (uint32_t)kWave >> ttl;
  const uint32_t qg = lane >> ttl;
  MaxSimTileWalk w;
  w.X = a.X;
  w.stride = a.stride;
  w.tnorm = a.tnorm;
  w.tile = lds + (size_t)qn * qst + (size_t)wib * tt * ld;
  w.d = a.d;
  w.ttl = ttl;
  w.ld = ld;
  w.metric = a.metric;
  w.lane = lane;
  const bool first_panel = a.panel_q0 == 0, last_panel = a.panel_q0 + qn >= a.nq;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;

  for (uint32_t i = blockIdx.x * kWavesPerBlock + wib; i < a.ndoc; i += total_waves) {
    const uint32_t t0 = a.doc_off[i], T = a.doc_cnt[i];  // (a document without vectors scores 0.0)
    float tot = first_panel ? 0.0f : a.total[i];
    int st = first_panel ? 0 : a.status[i];
    for (uint32_t g = 0; g < qn && T && !st; g += kQB * groups) {
      const uint32_t gq = g + qg * kQB;  // this lane's first query vector of the pass
      const float *qk[kQB];
      uint32_t qi[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) {
        qi[k] = gq + k < qn ? gq + k : qn - 1;
        qk[k] = qs + (size_t)qi[k] * qst;
      }
      float best[kQB];
      bool bad[kQB];
      maxsim_pass<OP, ORDER>(w, t0, T, g == 0, gq < qn, qk, a.qnorm + a.panel_q0, qi, best, bad);
      // the sum over query vectors: sequential, in query order -- group after group, each group's eight from its first
      // lane -- and the reference's error at the first query vector that has one (wave-uniform)
      for (uint32_t h = 0; h < groups; ++h) {
#pragma unroll
        for (int k = 0; k < kQB; ++k) {
          const float b = __shfl(best[k], (int)(h << ttl), kWave);
          const int f = __shfl(bad[k] ? 1 : 0, (int)(h << ttl), kWave);
          if (g + h * kQB + k < qn) add_query_max(b, f != 0, tot, st);
        }
      }
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

// Compaction of a store's slab (host/vt_mvstore.h): row j of the new slab and of the new norm column is row src[j] of
// the old ones -- order kept, 16 bytes per thread.
__global__ void mv_compact_kernel(const float *X, const double *norms, const uint32_t *src, uint32_t rows, uint32_t rs4,
                                  float *outX, double *out_norms) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (size_t)rows * rs4) return;
  const uint32_t j = (uint32_t)(u / rs4), c = (uint32_t)(u % rs4);
  const uint32_t s = src[j];
  reinterpret_cast<f32x4 *>(outX)[u] = reinterpret_cast<const f32x4 *>(X)[(size_t)s * rs4 + c];
  if (c == 0) out_norms[j] = norms[s];
}

template <int OP, int ORDER>
hipError_t launch_t(const MaxSimArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s) {
  auto kern = maxsim_resident_kernel<OP, ORDER>;
  const size_t lds = maxsim_resident_lds_bytes(a.panel_qn, a.q_stride, p);
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a, p.tile_log2, p.ld);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

bool maxsim_resident_plan(uint32_t d, uint32_t nq, int metric, MaxSimResidentPlan *out) {
  if (nq == 0 || metric == dev::M_HAM || metric == dev::M_JAC) return false;
  MaxSimResidentPlan p{};
  const uint32_t rs = dev::round_up(d, 4);
  p.ld = (rs / 4) % 2 ? rs : rs + 4;  // ld / 4 odd: one column of 64 rows is 64 different 16-byte banks
  p.q_stride = dev::round_up(d, 8);
  // as many query groups side by side as the call has use for, fewer rows per tile when the tiles would not fit
  p.tile_log2 = nq <= 8 ? 6 : nq <= 16 ? 5 : 4;
  const size_t qrow = (size_t)p.q_stride * sizeof(float);
  for (;; --p.tile_log2) {
    const size_t tiles = (size_t)kWavesPerBlock * ((size_t)1 << p.tile_log2) * p.ld * sizeof(float);
    const uint32_t pass = 8u * (64u >> p.tile_log2);  // query vectors of one pass: a panel holds whole passes
    if (tiles + (size_t)pass * qrow <= dev::kResidentLds) {
      const size_t fit = (dev::kResidentLds - tiles) / qrow / pass * pass;
      p.panel = (uint32_t)std::min<size_t>(fit, dev::round_up(nq, pass));
      break;
    }
    if (p.tile_log2 == 4) return false;  // (K9 serves such a dimension)
  }
  *out = p;
  return true;
}

size_t maxsim_resident_lds_bytes(uint32_t panel_qn, uint32_t q_stride, const MaxSimResidentPlan &p) {
  return ((size_t)panel_qn * q_stride + (size_t)kWavesPerBlock * ((size_t)1 << p.tile_log2) * p.ld) * sizeof(float);
}

hipError_t launch_maxsim_resident(const MaxSimArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s) {
  using namespace dev;
  // (no counts: float Hamming / Jaccard are K9's over the slab)
  return dispatch_pair<kPairF32 | kPairCos>(a.metric, a.order,
                                            [&](auto op, auto order) { return launch_t<op(), order()>(a, p, blocks, s); });
}

hipError_t launch_mv_compact(const float *X, const double *norms, const uint32_t *src, uint32_t rows, uint32_t stride,
                             float *outX, double *out_norms, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const size_t units = (size_t)rows * (stride / 4);
  hipLaunchKernelGGL(dev::mv_compact_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, X, norms, src, rows,
                     stride / 4, outX, out_norms);
  return hipGetLastError();
}

}  // namespace vt

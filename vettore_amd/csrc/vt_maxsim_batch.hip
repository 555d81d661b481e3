// vt_maxsim_batch.hip -- K9rb: K9r (vt_maxsim_resident.hip) for many query sets in one launch (gfx950).
//
// The query vectors of all sets lie in one matrix of slots: every set padded to whole groups of eight slots (the pad
// rows zero), so a lane's eight query vectors never straddle two sets.  A panel is a run of such groups -- whole sets --
// that fits in LDS beside the wave tiles; blockIdx.y picks a (panel, document list) pair, blockIdx.x strides the list's
// documents, one wave per document.  The wave stages the document's rows into its tile exactly as K9r does
// (vt_maxsim_pair.cuh is the pass they share: same chains, same tree maximum) and walks the panel's groups 64 / tt at
// a time.  What differs is the sum over query vectors: one descriptor per group says which set it belongs to, how many
// of its eight slots are real, and whether it is the set's first or last group.  Total and status start afresh at a
// set's first group -- nothing of a failed or overflowing set reaches the next --, live in registers across the passes
// of a long set, and leave at the set's last group: key and payload at keys[set * key_stride + i], or the set's own
// error word.  Pad slots are never summed and never looked at for an error.
#include "vt_maxsim_pair.cuh"

namespace vt {
namespace dev {

namespace {

template <int OP, int ORDER>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void maxsim_batch_kernel(const MaxSimBatchArgs a, const uint32_t ttl,
                                                                            const uint32_t ld) {
  extern __shared__ __align__(16) float lds[];  // [ndesc * 8][q_stride], then per wave [tt][ld]
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const MaxSimBatchGroup grp = a.groups[blockIdx.y];
  const uint32_t ndesc = grp.ndesc, qst = a.q_stride;
  const uint32_t slot0 = grp.desc0 * kQB, qn = ndesc * kQB;
  float *qs = lds;
  stage_query_panel(qs, a.Q + (size_t)slot0 * qst, qn * qst / 4);
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
  const MaxSimBatchDesc *desc = a.desc + grp.desc0;
  const uint32_t *doc_first = a.doc_first + grp.list0, *doc_cnt = a.doc_cnt + grp.list0, *doc_rank = a.doc_rank + grp.list0;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;

  for (uint32_t i = blockIdx.x * kWavesPerBlock + wib; i < grp.ndoc; i += total_waves) {
    const uint32_t t0 = doc_first[i], T = doc_cnt[i];  // (a document without vectors scores 0.0)
    float tot = 0.0f;
    int st = 0;
    for (uint32_t g = 0; g < ndesc; g += groups) {
      const uint32_t gi = g + qg;                        // this lane's group of the pass
      const uint32_t gc = gi < ndesc ? gi : ndesc - 1;   // (a lane past the panel's last group stays inside the panel)
      const float *qk[kQB];
      uint32_t qi[kQB];
#pragma unroll
      for (int k = 0; k < kQB; ++k) {
        qi[k] = gc * kQB + k;
        qk[k] = qs + (size_t)qi[k] * qst;
      }
      float best[kQB];
      bool bad[kQB];
      if (T) maxsim_pass<OP, ORDER>(w, t0, T, g == 0, gi < ndesc, qk, a.qnorm + slot0, qi, best, bad);
      // the sum over query vectors, set after set: sequential and in query order within a set, as in K9r
      for (uint32_t h = 0; h < groups && g + h < ndesc; ++h) {
        const MaxSimBatchDesc ds = desc[g + h];
        const uint32_t nlive = ds.info & 0xFFu;
        if (ds.info & kMaxSimBatchFirst) {
          tot = 0.0f;
          st = 0;
        }
        if (T) {
#pragma unroll
          for (int k = 0; k < kQB; ++k) {
            const float b = __shfl(best[k], (int)(h << ttl), kWave);
            const int f = __shfl(bad[k] ? 1 : 0, (int)(h << ttl), kWave);
            if ((uint32_t)k < nlive) add_query_max(b, f != 0, tot, st);
          }
        }
        if (!(ds.info & kMaxSimBatchLast) || lane != 0) continue;
        const size_t at = (size_t)ds.set * a.key_stride + i;
        write_document(a.keys + at, a.pay + at, a.first_error + ds.set, i, doc_rank + i, tot, st);
      }
    }
  }
}

template <int OP, int ORDER>
hipError_t launch_t(const MaxSimBatchArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s) {
  auto kern = maxsim_batch_kernel<OP, ORDER>;
  const size_t lds = maxsim_resident_lds_bytes(a.max_ndesc * kQB, a.q_stride, p);
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(blocks, a.ngroups), dim3(kWavesPerBlock * kWave), lds, s, a, p.tile_log2, p.ld);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

hipError_t launch_maxsim_batch(const MaxSimBatchArgs &a, const MaxSimResidentPlan &p, uint32_t blocks, hipStream_t s) {
  using namespace dev;
  if (a.ngroups == 0 || a.ngroups > 65535 || blocks == 0 || a.max_ndesc == 0 || a.q_stride != p.q_stride ||
      maxsim_resident_lds_bytes(a.max_ndesc * kQB, a.q_stride, p) > kResidentLds)
    return hipErrorInvalidValue;
  // (no counts: float Hamming / Jaccard take the single-set path)
  return dispatch_pair<kPairF32 | kPairCos>(a.metric, a.order,
                                            [&](auto op, auto order) { return launch_t<op(), order()>(a, p, blocks, s); });
}

}  // namespace vt

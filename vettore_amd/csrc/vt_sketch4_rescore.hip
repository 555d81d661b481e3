// vt_sketch4_rescore.hip -- K1n's last link: the candidates of the 4-bit pass rescored straight from the pass's
// lists, in the kernel that certifies them and finishes the search.  It stands where sketch_collect_kernel and the gathered
// K1 in filter mode (vt_scan_filter.hip) stood: no candidate array is written or read back, and a wave asks for several
// rows at once where K1's tile ring, built to stream, asked for eight rows in three dependent trips.
//
// One block per block of the pass; block b owns the lists [b * kSketch4BlockLists, + kSketch4BlockLists).
//   * Candidates: a slot is one iff its key(hi) word h != 0xffffffff and h <= Kt' (launch_sketch_refine's word) -- the
//     collect's rule.  Their rows go to LDS.  The certificate is the collect's too: a list whose kp slots are all candidates
//     raises the fail bit, the candidate total is kept exactly (on the word beside the ticket of the block's group: a
//     thousand blocks on one word would queue), ok = !fail && total <= cap.
//   * Rescoring: a wave per row with K1's arithmetic as sketch_refine_kernel has it -- lane l holds the floats
//     [256 s + 4 l, + 4) of segment s, elem4 / chunk_sum in the index's reduce order, the chunk sums to an LDS row, one lane
//     per row down the reference's sequential chain and the scalar tail.  A wave issues the loads of up to kRoundRows rows
//     (kRoundLoads one-KiB loads) before it waits for any; their chains are run by as many lanes at once.
//   * A row is kept iff it is valid by K1's rules and its rank word is <= Kt'; value, rank, finiteness, f64 recovery, status
//     word and key as scan_topk_kernel forms them.  Survivors, tickets and the finish are filter_claim / filter_finish of
//     vt_scan.cuh; the block that draws the last ticket also writes what the collect's last block wrote: info[1] = the
//     candidate total, info[2] = Kt', info[3] = 1, and info[0] = ok ? 2 : 0 unless it delivers.
//   * The word itself: *hi_word, or -- handed the pass's best words (Sketch4RescoreArgs::best_words: the exact keys of each
//     list's two best rows, left by the pass) -- their k-th smallest, Kt'', which every block finds for itself in its head
//     from words that lie in L2 (best_select); block 0 publishes it for the chain behind a second wait.  No launch stands
//     between the pass and this kernel then.
// Nothing polls or waits for another block.
#include "vt_scan.cuh"

namespace vt {
namespace dev {

constexpr uint32_t kRoundRows = 6;    // rows of a round at most: d <= 768 takes six, longer rows fewer
constexpr uint32_t kStaticSegs = 3;   // rows of up to three 1-KiB segments: an instantiation each, every slot's row and segment static
constexpr uint32_t kRoundLoads = kRoundRows * kStaticSegs;  // 1-KiB loads in flight at most: 72 VGPRs, four blocks a CU stay resident
constexpr uint32_t kLongLoads = 12;   // longer rows: the slots' rows and segments are run-time values, fewer fit the registers
constexpr uint32_t kFailBit = 2u;     // in fsync[1], beside the survivor list's overflow bit

// (rows per round for rows of `nseg` 1-KiB segments, nseg <= kLongLoads)
__host__ __device__ inline uint32_t rescore_round_rows(uint32_t nseg) {
  const uint32_t r = (nseg <= kStaticSegs ? kRoundLoads : kLongLoads) / nseg;
  return r < kRoundRows ? r : kRoundRows;
}

constexpr uint32_t kBestPer = kSketch4BestMaxWords / (kWavesPerBlock * kWave);  // best words a thread holds

// Kt'' (vt_device.h, Sketch4RescoreArgs::best_words): the k-th smallest of the block's 256 x kBestPer words with multiplicity,
// v[] this thread's (0xffffffff: an empty word, or none).  Exact, by counting: U = the k-th smallest of the threads' minima
// is the word of k distinct places, so Kt'' <= U, and a word below U lies with a thread whose minimum is below U -- fewer
// than k threads, at most 16 (k - 1) <= 256 words (k <= kSketch4BestMaxK): they are filed a word per thread, and Kt'' is
// their k-th smallest where they number k or more, U otherwise.  With fewer than k live words the k-th smallest is an empty
// word: the open threshold.  Called by the whole block, every block alike: no block reads another's.
__device__ __forceinline__ uint32_t best_select(const uint32_t (&v)[kBestPer], uint32_t k, uint32_t tid) {
  __shared__ __align__(16) uint32_t s_w[kWavesPerBlock * kWave];
  __shared__ uint32_t s_u, s_kt, s_below;
  static_assert(16 * (kSketch4BestMaxK - 1) <= kWavesPerBlock * kWave && kBestPer == 16, "the words below U fit a word per thread");
  uint32_t mine = 0xffffffffu;
#pragma unroll
  for (uint32_t u = 0; u < kBestPer; ++u) mine = v[u] < mine ? v[u] : mine;
  s_w[tid] = mine;
  if (tid == 0) s_below = 0;
  __syncthreads();
  auto place = [&](uint32_t x, uint32_t count, uint32_t *out) {  // *out = x where x is the k-th smallest of s_w[0..count)
    uint32_t lt = 0, le = 0;
    for (uint32_t j = 0; j < count; j += 4) {
      const uint4 o = *reinterpret_cast<const uint4 *>(s_w + j);
      lt += (o.x < x ? 1u : 0u) + (j + 1 < count && o.y < x ? 1u : 0u) + (j + 2 < count && o.z < x ? 1u : 0u) + (j + 3 < count && o.w < x ? 1u : 0u);
      le += (o.x <= x ? 1u : 0u) + (j + 1 < count && o.y <= x ? 1u : 0u) + (j + 2 < count && o.z <= x ? 1u : 0u) + (j + 3 < count && o.w <= x ? 1u : 0u);
    }
    if (lt < k && k <= le) *out = x;  // (every thread that gets here writes the same word)
  };
  place(mine, kWavesPerBlock * kWave, &s_u);
  __syncthreads();
  const uint32_t ub = s_u;
  if (mine < ub) {
#pragma unroll
    for (uint32_t u = 0; u < kBestPer; ++u)
      if (v[u] < ub) s_w[atomicAdd(&s_below, 1u)] = v[u];
  }
  __syncthreads();
  const uint32_t below = s_below;
  if (below < k) return ub;
  if (tid < below) place(s_w[tid], below, &s_kt);
  __syncthreads();
  return s_kt;
}

// NSEG: segments per row, 0: a.ld says (more than kStaticSegs)
template <int ORDER, int NSEG>
__global__ __launch_bounds__(kWavesPerBlock *kWave, 4) void sketch4_rescore_kernel(const Sketch4RescoreArgs a) {
  extern __shared__ __align__(16) float lds[];  // the query | the waves' chunk sums [waves][rows][ss] | candidate rows | list counts
  __shared__ uint32_t s_n;
  const ScanArgs &f = a.s;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int odd = lane & 1;
  constexpr uint32_t kLoads = NSEG ? kRoundRows * NSEG : kLongLoads;
  const uint32_t nseg = NSEG ? (uint32_t)NSEG : (a.ld + 255u) / 256u, rr = rescore_round_rows(nseg);
  float *S = lds + a.ld + (uint32_t)wib * (rr * a.ss);
  uint32_t *stage = reinterpret_cast<uint32_t *>(lds + a.ld + kWavesPerBlock * (rr * a.ss));
  uint32_t *lcnt = stage + kSketch4BlockLists * a.kp;

  // One trip to memory for everything the block needs before it can ask for a row: its slots' words and rows (a thread per
  // slot: kp <= kSmallK), the threshold word -- an earlier launch wrote all three: plain loads -- and the query.
  static_assert(kSketch4BlockLists * kSmallK <= kWavesPerBlock * kWave, "a thread per slot");
  const uint32_t slots = kSketch4BlockLists * a.kp, first = blockIdx.x * slots;
  const uint32_t h = tid < slots ? a.hi_words[first + tid] : 0xffffffffu;
  const uint32_t row = tid < slots ? a.pay[first + tid].row : 0u;  // (an empty slot's payload was never written: loaded, not used)
  // (the threshold from the pass's best rows: their words ride in the same trip, sixteen a thread, four loads of 16 bytes
  // where four words are there)
  uint32_t bw[kBestPer];
#pragma unroll
  for (uint32_t u = 0; u < kBestPer; ++u) bw[u] = 0xffffffffu;
  if (a.best_words) {
#pragma unroll
    for (uint32_t j = 0; j < kBestPer / 4; ++j) {
      const uint32_t at = (j * blockDim.x + tid) * 4u;
      if (at + 4u <= a.best_count) {
        const uint4 w = *reinterpret_cast<const uint4 *>(a.best_words + at);
        bw[4 * j] = w.x;
        bw[4 * j + 1] = w.y;
        bw[4 * j + 2] = w.z;
        bw[4 * j + 3] = w.w;
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
          if (at + e < a.best_count) bw[4 * j + e] = a.best_words[at + e];
      }
    }
  }
  uint32_t kt = a.best_words ? 0u : *f.hi_word;
  for (uint32_t i = tid; i < a.ld; i += blockDim.x) lds[i] = f.q[i];
  if (tid < kSketch4BlockLists) lcnt[tid] = 0;
  if (tid == 0) {
    s_n = 0;
    *filter_stored_flag() = 0;
  }
  __syncthreads();
  if (a.best_words) {  // (the head: before any row is asked for)
    kt = best_select(bw, f.k, tid);
    if (blockIdx.x == 0 && tid == 0) *a.kt_out = kt;
  }

  // the block's own lists: candidates' rows to LDS, each list's count
  {  // (whole waves: the claim votes)
    const uint32_t i = tid;
    const bool cand = h != 0xffffffffu && h <= kt;
    const uint64_t act = __ballot(cand);
    if (act) {
      const int leader = __ffsll((long long)act) - 1;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&s_n, (uint32_t)__popcll(act));
      base = (uint32_t)__shfl((int)base, leader, kWave);
      if (cand) {
        stage[base + (uint32_t)__popcll(act & ((1ull << lane) - 1ull))] = row;
        atomicAdd(&lcnt[i / a.kp], 1u);
      }
    }
  }
  __syncthreads();
  const uint32_t n = s_n;
  const uint32_t groups = gridDim.x < kScanFilterGroups ? gridDim.x : kScanFilterGroups;
  if (tid == 0 && n) filter_agent_add(f.fsync + kScanFilterLine * (1 + blockIdx.x % groups) + 1, n);
  if (tid < kSketch4BlockLists && lcnt[tid] == a.kp)
    __hip_atomic_fetch_or(f.fsync + 1, kFailBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  // K1 on the candidates: wave w takes candidates w, w + 4, ..., up to rr of them a round
  const uint32_t cfull = f.d / 8, tail = f.d % 8, tail_base = a.ss - 12;
  const uint32_t nw = n > (uint32_t)wib ? (n - (uint32_t)wib + kWavesPerBlock - 1) / kWavesPerBlock : 0u;
  const uint32_t l4 = (uint32_t)lane * 4u;
  const int order = ORDER >= 0 ? ORDER : f.order;
  for (uint32_t i0 = 0; i0 < nw; i0 += rr) {
    const uint32_t left = nw - i0 < rr ? nw - i0 : rr;  // rows of this round, >= 1
    const bool chain = (uint32_t)lane < left;
    const uint32_t my_row = stage[(uint32_t)wib + kWavesPerBlock * (i0 + (chain ? (uint32_t)lane : 0u))];
    uint32_t my_rank = my_row;
    if (chain && f.id_rank) my_rank = f.id_rank[my_row];

    // every load of the round, then every product.  A slot past the round's rows, and a lane past the row's end, loads
    // what another slot or lane loads: nothing is asked for conditionally, nothing of it is used
    f32x4 x[kLoads];
    {
      uint32_t r = 0, s = 0;
#pragma unroll
      for (uint32_t j = 0; j < kLoads; ++j) {
        const uint32_t ru = r < left ? r : 0u;
        const uint32_t src = (uint32_t)__builtin_amdgcn_readlane((int)my_row, (int)ru);
        const uint32_t col = s * 256u + l4, colc = col < a.ld ? col : a.ld - 4u;
        x[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(f.X + (size_t)src * f.stride + colc));
        if (++s == nseg) {
          s = 0;
          r = r + 1 < rr ? r + 1 : r;  // (past the last row: the slots left repeat its last segment)
        }
      }
    }
    {
      uint32_t r = 0, s = 0;
      bool live = true;
#pragma unroll
      for (uint32_t j = 0; j < kLoads; ++j) {
        const uint32_t col = s * 256u + l4, colc = col < a.ld ? col : a.ld - 4u;
        const f32x4 qv = *reinterpret_cast<const f32x4 *>(lds + colc);
        const f32x4 pr = elem4<OP_DOT>(OP_DOT, qv, x[j]);
        const float sum = chunk_sum<OP_DOT, ORDER>(OP_DOT, order, pr.x, pr.y, pr.z, pr.w, odd);
        const uint32_t ch = col >> 3;
        float *Srow = S + r * a.ss;
        if (live && r < left && col < a.ld) {
          if (ch < cfull) {
            if (!odd) Srow[ch] = sum;
          } else if (ch == cfull) {  // the tail chunk: the reference adds these products one by one
            *reinterpret_cast<f32x4 *>(Srow + tail_base + odd * 4) = pr;
          }
        }
        if (++s == nseg) {
          s = 0;
          if (r + 1 < rr) r = r + 1;
          else live = false;
        }
      }
    }
    wave_lds_fence();

    // lane r continues row r's sequential chain
    float acc = 0.0f;
    if (chain) {
      const float *Sr = S + (uint32_t)lane * a.ss;
      uint32_t c = 0;
      // (a batch of the row's sums is read before the first of them is added: the adds depend on one another, the reads
      // do not, and one at a time each add would wait for its own LDS read)
      constexpr uint32_t kBatch = 12;
      for (; c + 4 * kBatch <= cfull; c += 4 * kBatch) {
        f32x4 v[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) v[j] = *reinterpret_cast<const f32x4 *>(Sr + c + 4 * j);
#pragma unroll
        for (uint32_t j = 0; j < kBatch; ++j) {
          acc = acc + v[j].x;
          acc = acc + v[j].y;
          acc = acc + v[j].z;
          acc = acc + v[j].w;
        }
      }
      for (; c + 4 <= cfull; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(Sr + c);
        acc = acc + v.x;
        acc = acc + v.y;
        acc = acc + v.z;
        acc = acc + v.w;
      }
      for (; c < cfull; ++c) acc = acc + Sr[c];
      for (uint32_t j = 0; j < tail; ++j) acc = acc + Sr[tail_base + j];
    }
    wave_lds_fence();
    // distances.rs:42-68 compute(): value, finiteness, f64 recovery -- as scan_topk_kernel has them
    const int metric = f.metric;
    float raw = metric == M_NIP ? -acc : acc;
    bool valid = chain;
    if (valid && !finite_f32(raw)) {
      const float rec = recover_overflow(metric, f.q, f.X + (size_t)my_row * f.stride, f.d);
      if (rec == rec) {
        raw = rec;
      } else {
        atomicMax(f.status, kErrOverflow);
        valid = false;
      }
    }
    // distances.rs:113-119 rank_value, flat.rs:34-40 ordering
    float rank = raw;
    if (metric == M_COS) rank = 1.0f - raw;
    else if (metric == M_IP) rank = -raw;
    const uint64_t key = ((uint64_t)orderable(rank) << 32) | my_rank;
    const bool keep = valid && (uint32_t)(key >> 32) <= kt;
    const uint32_t pos = filter_claim(f.fsync + 0, keep, lane);
    if (keep) {
      if (pos < f.surv_cap) {
        *filter_stored_flag() = 1;
        f.surv_keys[pos] = key;
        Payload pv;
        pv.row = my_row;
        pv.raw = raw;
        f.surv_pay[pos] = pv;
      } else {
        __hip_atomic_fetch_or(f.fsync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  // the finish; the lane with the last ticket reads the survivor count, the overflow / fail word and the groups' candidate
  // totals in one trip (every block's adds are behind its ticket; agent-scope atomic loads alone, as the finish reads the
  // entries) and writes the certificate where the collect's last block wrote it
  filter_finish(f, 1u, gridDim.x, filter_stored_flag(), [&](uint32_t *nsurv) {
    const uint32_t ns = __hip_atomic_load(f.fsync + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t over = __hip_atomic_load(f.fsync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t part[kScanFilterGroups];
#pragma unroll
    for (uint32_t g = 0; g < kScanFilterGroups; ++g)
      part[g] = g < groups ? __hip_atomic_load(f.fsync + kScanFilterLine * (1 + g) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    uint32_t total = 0;
#pragma unroll
    for (uint32_t g = 0; g < kScanFilterGroups; ++g) total += part[g];
    const bool ok = !(over & kFailBit) && total <= a.cap;
    f.info[0] = ok ? 2u : 0u;
    f.info[1] = total;
    f.info[2] = kt;
    f.info[3] = 1u;
    *nsurv = ns;
    return ok && !over && ns <= f.surv_cap;
  });
}

template <int ORDER, int NSEG>
static hipError_t launch_rescore_t(const Sketch4RescoreArgs &a, uint32_t blocks, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((sketch4_rescore_kernel<ORDER, NSEG>), dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}
template <int ORDER>
static hipError_t launch_rescore_segs(const Sketch4RescoreArgs &a, uint32_t blocks, size_t lds, hipStream_t s) {
  static_assert(kStaticSegs == 3, "an instantiation per static segment count");
  const uint32_t nseg = (a.ld + 255u) / 256u;
  if (nseg == 1) return launch_rescore_t<ORDER, 1>(a, blocks, lds, s);
  if (nseg == 2) return launch_rescore_t<ORDER, 2>(a, blocks, lds, s);
  if (nseg == 3) return launch_rescore_t<ORDER, 3>(a, blocks, lds, s);
  return launch_rescore_t<ORDER, 0>(a, blocks, lds, s);
}
}  // namespace dev

using namespace dev;

size_t sketch4_rescore_lds_bytes(uint32_t d, uint32_t kp) {
  if (d == 0 || kp == 0 || kp > (uint32_t)kSmallK) return 0;
  const uint32_t ld = padded_dim(d), nseg = (ld + 255u) / 256u;
  if (nseg > kLongLoads) return 0;
  const size_t ss = ld / 8 + 12;  // (K1's panel row: 4 * odd dwords, the eight tail products behind the sums)
  const size_t bytes = ((size_t)ld + (size_t)kWavesPerBlock * rescore_round_rows(nseg) * ss + (size_t)kSketch4BlockLists * kp + 4) * 4;
  // four blocks a CU: the finish keeps kScanFilterCap keys and payloads in static LDS beside these (16 KiB)
  return bytes <= kMaxLds / 4 - 18 * 1024 ? bytes : 0;
}

hipError_t launch_sketch4_rescore(Sketch4RescoreArgs a, uint32_t blocks, hipStream_t s) {
  const ScanArgs &f = a.s;
  const size_t lds = sketch4_rescore_lds_bytes(f.d, a.kp);
  if (!lds || blocks == 0 || f.k == 0 || f.k > (uint32_t)kSmallK || f.k > a.kp || metric_op(f.metric) != OP_DOT || f.has_lo ||
      f.stride < padded_dim(f.d) || !f.X || !f.q || !a.hi_words || !a.pay || (!f.hi_word && !a.best_words) || !f.surv_keys ||
      !f.surv_pay || f.surv_cap == 0 || f.surv_cap > kScanFilterCap || !f.fsync || !f.out || !f.info || !f.status)
    return hipErrorInvalidValue;
  if (a.best_words && (a.best_count == 0 || a.best_count > kSketch4BestMaxWords || f.k > kSketch4BestMaxK || !a.kt_out ||
                       reinterpret_cast<uintptr_t>(a.best_words) % 16))
    return hipErrorInvalidValue;
  a.ld = padded_dim(f.d);
  a.ss = a.ld / 8 + 12;
  if (f.order == kDefaultReduceOrder) return launch_rescore_segs<kDefaultReduceOrder>(a, blocks, lds, s);
  return launch_rescore_segs<-1>(a, blocks, lds, s);
}

}  // namespace vt

// vt_select.hip -- K3 (gfx950): the k best of a key list, sorted -- one block's radix select, the spread form for a
// funnel group's lists, the rank sort of a whole short list, the cross-shard merge -- and the exact k-th key of a
// whole key column for limits above kMaxFusedK.  Each kernel is followed by its launchers.
#include "vt_scan.cuh"

namespace vt {

using namespace dev;

namespace {

// ---------------------------------------------------------------------------
// K3: top-k of the partial lists, sorted ascending.  Replaces `hits.sort()`
// (flat.rs:120-121, search.rs:107-110) and the cross-wave merge the reference's
// single heap never needed.  One 1024-thread block, MSD radix select on the u64
// keys with 8-bit digits starting at the highest bit in which the keys differ:
//   pass 1  range + count of the live keys,
//   pass 2  histogram of the first digit -> the bin holding the k-th key,
//   pass 3  keys below that bin are winners; keys in it move to an LDS list,
//   then the remaining digits are resolved on the LDS list only.
// Keys are distinct when every row carries its own id rank; rows that share the lazy
// mode's sentinel rank (and callers' duplicate ids) can carry EQUAL keys, so "<= threshold"
// may hold more than k: everything below the threshold is filed first, then its equals, and
// only equals are ever left out.  The winners are rank-sorted in LDS and written, with the
// status word of the scan, straight into the host-mapped result block.
// ---------------------------------------------------------------------------
constexpr uint32_t kSelCand = 4096;  // LDS candidate list capacity

struct SelectBin {
  uint32_t bin, below, count;
};

// Finds the histogram bin containing the krem-th smallest (1-based); wave 0 only.
__device__ __forceinline__ void select_find_bin(const uint32_t *hist, uint32_t krem, int lane, SelectBin *out) {
  const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
  const uint32_t mine = h0 + h1 + h2 + h3;
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  const uint32_t excl = incl - mine;
  if (excl < krem && krem <= incl) {
    uint32_t below = excl, b = 4 * lane, c = h0;
    if (below + c < krem) {
      below += c; b += 1; c = h1;
      if (below + c < krem) {
        below += c; b += 1; c = h2;
        if (below + c < krem) { below += c; b += 1; c = h3; }
      }
    }
    out->bin = b;
    out->below = below;
    out->count = c;
  }
}

// Visits keys[i] for i = tid, tid + 1024, ... with 8 independent loads in flight
// per thread (one block has to stream up to a few MB out of L2 by itself).
template <typename F>
__device__ __forceinline__ void for_each_key(const uint64_t *__restrict__ keys, uint32_t m, uint32_t tid, F f) {
  constexpr uint32_t kStride = 1024, kUnroll = 8;
  uint32_t i = tid;
  for (; i + (kUnroll - 1) * kStride < m; i += kUnroll * kStride) {
    uint64_t v[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) v[u] = keys[i + u * kStride];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) f(v[u], i + u * kStride);
  }
  for (; i < m; i += kStride) f(keys[i], i);
}

// With more than one block (first level of a two-level select over a long
// list) block b works on its own slice of `slice` keys and leaves its winners,
// unsorted and padded with kEmptyKey, at part_keys/part_pay[b * k ..).
__global__ __launch_bounds__(1024) void select_topk_kernel(const uint64_t *__restrict__ keys,
                                                           const Payload *__restrict__ pay, uint32_t m, uint32_t k,
                                                           uint64_t lo_key, int has_lo, int *dev_status,
                                                           ResultBlock *out, uint32_t slice,
                                                           uint64_t *__restrict__ part_keys,
                                                           Payload *__restrict__ part_pay,
                                                           const uint32_t *__restrict__ m_dev, uint32_t out_stride,
                                                           uint32_t skip_upto = 0) {
  extern __shared__ __align__(16) unsigned char smem[];
  const uint32_t m_stride = m;
  // list length decided on the device (hamming_collect_kernel): one count per query
  if (m_dev) m = m_dev[blockIdx.y] < m ? m_dev[blockIdx.y] : m;
  if (m_dev && skip_upto && m <= skip_upto) return;  // (select_lists_spread_kernel, launched beside this one, takes those)
  if (gridDim.y > 1) {
    // one list of up to m keys per query (grid.y = queries): query y's winners go to the block
    // `out_stride` bytes after query y - 1's (header + k entries when packed tightly)
    keys += (size_t)blockIdx.y * m_stride;
    pay += (size_t)blockIdx.y * m_stride;
    out = reinterpret_cast<ResultBlock *>(reinterpret_cast<unsigned char *>(out) + (size_t)blockIdx.y * out_stride);
  }
  // part_keys != nullptr: the winners go, unsorted and padded with kEmptyKey, to
  // part_keys/part_pay[blockIdx.x * k ..) instead of a result block -- the first level of
  // a two-level select (several blocks, one slice each) or a device-resident list of up to
  // kSelListMax rows for a following stage (one block).
  const bool partial = part_keys != nullptr;
  if (gridDim.x > 1) {
    const uint32_t lo = blockIdx.x * slice;
    keys += lo;
    pay += lo;
    m = lo >= m ? 0u : (m - lo < slice ? m - lo : slice);
  }
  if (!partial && gridDim.x == 1 && m <= 1024) {
    // A short list -- the few hundred keys a threshold collect leaves, a candidate set being
    // reranked: one key per thread, its place found by counting the smaller ones.  None of
    // the radix passes' fixed cost (9-10 us -> ~3 us for 200 keys).
    uint64_t *sk = reinterpret_cast<uint64_t *>(smem);  // [1024] (the dynamic LDS holds 4096 + k keys)
    __shared__ uint32_t s_live;
    const uint32_t t = threadIdx.x;
    uint64_t key = kEmptyKey;
    if (t < m) {
      key = keys[t];
      if (has_lo && key <= lo_key) key = kEmptyKey;
    }
    sk[t] = key;
    if (t == 0) s_live = 0;
    __syncthreads();
    const bool alive = key != kEmptyKey;
    const uint64_t votes = __ballot(alive);
    if ((t & (kWave - 1)) == 0 && votes) atomicAdd(&s_live, (uint32_t)__popcll(votes));
    if (alive) {
      uint32_t pos = 0;
      for (uint32_t x = 0; x < m; ++x) {
        const uint64_t kx = sk[x];
        pos += (kx < key || (kx == key && x < t)) ? 1u : 0u;
      }
      if (pos < k) {
        const Payload p = pay[t];
        Entry e;
        e.key = key;
        e.row = p.row;
        e.raw = p.raw;
        out->e[pos] = e;
      }
    }
    __syncthreads();
    if (t == 0) {
      out->count = s_live < k ? s_live : k;
      out->status = dev_status ? *dev_status : 0;
      if (dev_status) *dev_status = 0;
    }
    return;
  }
  uint64_t *sel_key = reinterpret_cast<uint64_t *>(smem);  // [k]
  uint64_t *cand_key = sel_key + k;                        // [kSelCand]
  uint32_t *sel_idx = reinterpret_cast<uint32_t *>(cand_key + kSelCand);  // [k]
  uint32_t *cand_idx = sel_idx + k;                                       // [kSelCand]
  __shared__ uint32_t hist[256];
  __shared__ uint64_t red_min[16], red_max[16];
  __shared__ uint32_t red_cnt[16];
  __shared__ SelectBin s_bin;
  __shared__ uint32_t s_sel, s_ncand;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid >> 6;

  auto live = [&](uint64_t key) { return key != kEmptyKey && (!has_lo || key > lo_key); };

  // pass 1: count of the live keys and the bit positions in which they differ
  // (OR ^ AND): digits are cut from those positions only, so the long constant
  // runs of a key -- an id rank below 2^24 under a 32-bit score, the handful of
  // distinct Hamming distances -- cost no rounds
  uint64_t mn = ~0ull, mx = 0;  // AND, OR
  uint32_t cnt = 0;
  for_each_key(keys, m, tid, [&](uint64_t key, uint32_t) {
    if (live(key)) {
      mn &= key;
      mx |= key;
      cnt += 1;
    }
  });
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn &= __shfl_xor(mn, o, kWave);
    mx |= __shfl_xor(mx, o, kWave);
    cnt += __shfl_xor(cnt, o, kWave);
  }
  if (lane == 0) {
    red_min[wave] = mn;
    red_max[wave] = mx;
    red_cnt[wave] = cnt;
  }
  if (tid == 0) {
    s_sel = 0;
    s_ncand = 0;
  }
  if (tid < 256) hist[tid] = 0;
  __syncthreads();
  mn = ~0ull;
  mx = 0;
  uint32_t nvalid = 0;
  for (int w = 0; w < 16; ++w) {
    mn &= red_min[w];
    mx |= red_max[w];
    nvalid += red_cnt[w];
  }
  const uint64_t var = nvalid ? (mn ^ mx) : 0ull;  // bits that differ among the live keys

  uint64_t T = ~0ull - 1;  // threshold over the global keys: select every live key <= T
  bool from_cand = false;  // the remaining winners are cand keys <= Tc
  uint64_t Tc = 0;
  if (nvalid > k && var != 0) {
    uint32_t krem = k;
    int hb = 63 - __clzll((long long)var);
    uint64_t mask = ~var;          // constant bits count as resolved
    uint64_t prefix = mx & mask;
    int width = hb + 1 < 8 ? hb + 1 : 8;
    int shift = hb + 1 - width;
    uint32_t dmask = (1u << width) - 1;
    // highest varying bit below `shift`, or -1: the next digit starts there
    auto next_hb = [&](int sh) -> int {
      const uint64_t rem = sh > 0 ? (var & ((1ull << sh) - 1)) : 0ull;
      return rem ? 63 - __clzll((long long)rem) : -1;
    };
    // Threshold when the walk ends in the bin `prefix`.  The whole bin is selected (its count is what remained): the bin's
    // top.  Otherwise no varying bit is left below the digit and the bin holds more EQUAL keys than remain: their value is
    // `prefix` itself (the constant low bits are in it), and the threshold must be that value -- under the bin's top the
    // equals would pass "key < threshold" and race the strictly smaller keys for the k places.
    auto bin_threshold = [](uint64_t pfx, int sh, bool whole) -> uint64_t {
      return whole && sh ? (pfx | ((1ull << sh) - 1)) : pfx;
    };
    // pass 2: first digit
    for_each_key(keys, m, tid, [&](uint64_t key, uint32_t) {
      if (live(key)) atomicAdd(&hist[(uint32_t)(key >> shift) & dmask], 1u);
    });
    __syncthreads();
    if (wave == 0) select_find_bin(hist, krem, lane, &s_bin);
    __syncthreads();
    SelectBin sb = s_bin;
    krem -= sb.below;
    prefix |= (uint64_t)sb.bin << shift;
    mask |= (uint64_t)dmask << shift;
    if (sb.count == krem || next_hb(shift) < 0) {
      T = bin_threshold(prefix, shift, sb.count == krem);
    } else if (sb.count <= kSelCand) {
      // pass 3: winners below the bin, the bin itself into LDS
      const uint64_t bin_lo = prefix, bin_hi = prefix | ((1ull << shift) - 1);
      for_each_key(keys, m, tid, [&](uint64_t key, uint32_t i) {
        if (!live(key) || key > bin_hi) return;
        if (key < bin_lo) {
          const uint32_t pos = atomicAdd(&s_sel, 1u);
          if (pos < k) {
            sel_key[pos] = key;
            sel_idx[pos] = i;
          }
        } else {
          const uint32_t pos = atomicAdd(&s_ncand, 1u);
          if (pos < kSelCand) {
            cand_key[pos] = key;
            cand_idx[pos] = i;
          }
        }
      });
      __syncthreads();
      const uint32_t ncand = s_ncand < kSelCand ? s_ncand : kSelCand;
      // remaining digits on the LDS list
      hb = next_hb(shift);
      for (;;) {
        width = hb + 1 < 8 ? hb + 1 : 8;
        shift = hb + 1 - width;
        dmask = (1u << width) - 1;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < ncand; i += 1024) {
          const uint64_t key = cand_key[i];
          if ((key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & dmask], 1u);
        }
        __syncthreads();
        if (wave == 0) select_find_bin(hist, krem, lane, &s_bin);
        __syncthreads();
        sb = s_bin;
        krem -= sb.below;
        prefix |= (uint64_t)sb.bin << shift;
        mask |= (uint64_t)dmask << shift;
        if (sb.count == krem || next_hb(shift) < 0) {
          Tc = bin_threshold(prefix, shift, sb.count == krem);
          break;
        }
        hb = next_hb(shift);
      }
      from_cand = true;
      // (equal keys exist -- see WaveTopK::compact: everything below the threshold is filed
      // before its equals, so that only equals can be left out)
      for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t i = tid; i < ncand; i += 1024) {
          const uint64_t key = cand_key[i];
          if (pass == 0 ? key < Tc : key == Tc) {
            const uint32_t pos = atomicAdd(&s_sel, 1u);
            if (pos < k) {
              sel_key[pos] = key;
              sel_idx[pos] = cand_idx[i];
            }
          }
        }
        __syncthreads();
      }
    } else {
      // crowded bin (more than kSelCand keys share the digit): keep resolving on the global keys
      hb = next_hb(shift);
      for (;;) {
        width = hb + 1 < 8 ? hb + 1 : 8;
        shift = hb + 1 - width;
        dmask = (1u << width) - 1;
        __syncthreads();
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for_each_key(keys, m, tid, [&](uint64_t key, uint32_t) {
          if (live(key) && (key & mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & dmask], 1u);
        });
        __syncthreads();
        if (wave == 0) select_find_bin(hist, krem, lane, &s_bin);
        __syncthreads();
        sb = s_bin;
        krem -= sb.below;
        prefix |= (uint64_t)sb.bin << shift;
        mask |= (uint64_t)dmask << shift;
        if (sb.count == krem || next_hb(shift) < 0) {
          T = bin_threshold(prefix, shift, sb.count == krem);
          break;
        }
        hb = next_hb(shift);
      }
    }
  }

  if (!from_cand) {
    // compaction of the winners straight from the global keys: below the threshold first, then
    // its equals
    for (int pass = 0; pass < 2; ++pass) {
      for_each_key(keys, m, tid, [&](uint64_t key, uint32_t i) {
        if (live(key) && (pass == 0 ? key < T : key == T)) {
          const uint32_t pos = atomicAdd(&s_sel, 1u);
          if (pos < k) {
            sel_key[pos] = key;
            sel_idx[pos] = i;
          }
        }
      });
      __syncthreads();
    }
  }
  __syncthreads();
  const uint32_t nsel = s_sel < k ? s_sel : k;
  if (partial) {
    for (uint32_t j = tid; j < k; j += 1024) {
      part_keys[(size_t)blockIdx.x * k + j] = j < nsel ? sel_key[j] : kEmptyKey;
      Payload pad;  // padding entries must still be safe to gather from: row 0
      pad.row = 0;
      pad.raw = 0.0f;
      part_pay[(size_t)blockIdx.x * k + j] = j < nsel ? pay[sel_idx[j]] : pad;
    }
    return;
  }
  // rank sort (keys distinct; ties only for caller-supplied duplicate ids)
  for (uint32_t j = tid; j < nsel; j += 1024) {
    const uint64_t kj = sel_key[j];
    uint32_t pos = 0;
    for (uint32_t x = 0; x < nsel; ++x) {
      const uint64_t kx = sel_key[x];
      pos += (kx < kj || (kx == kj && x < j)) ? 1u : 0u;
    }
    const Payload p = pay[sel_idx[j]];
    Entry e;
    e.key = kj;
    e.row = p.row;
    e.raw = p.raw;
    out->e[pos] = e;
  }
  if (tid == 0) {
    out->count = nsel;
    // dev_status == nullptr: an intermediate stage -- the flag stays where it is
    // and reaches the host with the last select of the chain
    out->status = dev_status ? *dev_status : 0;
    if (dev_status) *dev_status = 0;
  }
}

// The k best of each query's list, for lists of up to kSpreadKeys keys, on kSpreadBlocks blocks per list (r05).  A key's
// place among the winners is the number of smaller keys -- computable for every key on its own -- so each block stages the
// whole list in LDS (one sweep of <= 16 KB) and places ITS 128 keys; nothing is exchanged between blocks.  Against the
// one-block forms above: counting on one block is m x m / 64 wave-iterations on ONE CU (60 us at 1 000 keys), the radix
// form four or five DEPENDENT sweeps of the keys in global memory -- 47 us alone, 0.6 ms beside another context's sweep
// of the corpus, which is where a funnel group's list select runs (profiles/r05_funnel64_trace_excerpt.txt).  Longer
// lists return at once: select_topk_kernel is launched beside this kernel with skip_upto = kSpreadKeys.
constexpr uint32_t kSpreadKeys = 2048, kSpreadBlocks = 16, kSpreadThreads = kSpreadKeys / kSpreadBlocks;
__global__ __launch_bounds__(kSpreadThreads) void select_lists_spread_kernel(const uint64_t *__restrict__ keys,
                                                                            const Payload *__restrict__ pay, uint32_t m_stride,
                                                                            const uint32_t *__restrict__ m_dev, uint32_t k,
                                                                            ResultBlock *out, uint32_t out_stride) {
  __shared__ uint64_t sk[kSpreadKeys];
  __shared__ uint32_t s_live;
  const uint32_t y = blockIdx.y;
  const uint32_t m = m_dev[y] < m_stride ? m_dev[y] : m_stride;
  if (m > kSpreadKeys) return;
  keys += (size_t)y * m_stride;
  pay += (size_t)y * m_stride;
  out = reinterpret_cast<ResultBlock *>(reinterpret_cast<unsigned char *>(out) + (size_t)y * out_stride);
  const uint32_t t = threadIdx.x;
  if (t == 0) s_live = 0;
  for (uint32_t i = t; i < m; i += kSpreadThreads) sk[i] = keys[i];
  __syncthreads();
  if (blockIdx.x == 0) {  // the list's header
    uint32_t live = 0;
    for (uint32_t i = t; i < m; i += kSpreadThreads) live += sk[i] != kEmptyKey ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) live += __shfl_xor(live, o, kWave);
    if ((t & (kWave - 1)) == 0) atomicAdd(&s_live, live);
    __syncthreads();
    if (t == 0) {
      out->count = s_live < k ? s_live : k;
      out->status = 0;  // (an intermediate stage: the overflow flag reaches the host with the chain's last select)
    }
  }
  const uint32_t i = blockIdx.x * kSpreadThreads + t;
  const uint64_t key = i < m ? sk[i] : kEmptyKey;
  if (__ballot(key != kEmptyKey) == 0) return;  // (wave-uniform: a wave without keys does not walk the list)
  uint32_t pos = 0;
  for (uint32_t x = 0; x < m; ++x) {
    const uint64_t kx = sk[x];
    pos += (kx < key || (kx == key && x < i)) ? 1u : 0u;
  }
  if (key != kEmptyKey && pos < k) {
    const Payload p = pay[i];
    Entry e;
    e.key = key;
    e.row = p.row;
    e.raw = p.raw;
    out->e[pos] = e;
  }
}

}  // namespace

hipError_t launch_select(const uint64_t *keys, const Payload *pay, uint32_t m, uint32_t k, uint64_t lo_key, int has_lo,
                         int *dev_status, ResultBlock *out, uint64_t *scratch_keys, Payload *scratch_pay,
                         hipStream_t s, const uint32_t *m_dev) {
  if (k == 0 || k > (uint32_t)kMaxFusedK) return hipErrorInvalidValue;
  const size_t lds = ((size_t)k + kSelCand) * 12;
  if (m >= kSelTwoLevelMin && scratch_keys && scratch_pay && !m_dev) {
    // long lists (k = 100 leaves 51 200 partial keys): kSelGroups blocks select in
    // parallel on slices, one block finishes on kSelGroups * k keys
    const uint32_t slice = (m + kSelGroups - 1) / kSelGroups;
    hipLaunchKernelGGL(select_topk_kernel, dim3(kSelGroups), dim3(1024), lds, s, keys, pay, m, k, lo_key, has_lo,
                       dev_status, out, slice, scratch_keys, scratch_pay, nullptr, 0u);
    hipLaunchKernelGGL(select_topk_kernel, dim3(1), dim3(1024), lds, s, scratch_keys, scratch_pay, kSelGroups * k, k,
                       0ull, 0, dev_status, out, 0u, nullptr, nullptr, nullptr, 0u);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(select_topk_kernel, dim3(1), dim3(1024), lds, s, keys, pay, m, k, lo_key, has_lo, dev_status, out,
                     0u, nullptr, nullptr, m_dev, 0u);
  return hipGetLastError();
}

hipError_t launch_select_list(const uint64_t *keys, const Payload *pay, uint32_t m, const uint32_t *m_dev, uint32_t k,
                              uint64_t *out_keys, Payload *out_pay, hipStream_t s) {
  if (k == 0 || k > kSelListMax || !out_keys || !out_pay) return hipErrorInvalidValue;
  const size_t lds = ((size_t)k + kSelCand) * 12;
  hipError_t e = allow_lds(select_topk_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_topk_kernel, dim3(1), dim3(1024), lds, s, keys, pay, m, k, 0ull, 0, nullptr, nullptr, 0u,
                     out_keys, out_pay, m_dev, 0u);
  return hipGetLastError();
}

hipError_t launch_select_queries(const uint64_t *keys, const Payload *pay, uint32_t nq, uint32_t m, uint32_t k, void *out,
                                 uint32_t out_stride, hipStream_t s) {
  if (k == 0 || k > (uint32_t)kMaxFusedK || nq == 0 || nq > 65535 || out_stride < 16 + k * sizeof(Entry) || out_stride % 16)
    return hipErrorInvalidValue;
  const size_t lds = ((size_t)k + kSelCand) * 12;
  hipError_t e = allow_lds(select_topk_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_topk_kernel, dim3(1, nq), dim3(1024), lds, s, keys, pay, m, k, 0ull, 0, nullptr,
                     static_cast<ResultBlock *>(out), 0u, nullptr, nullptr, nullptr, out_stride);
  return hipGetLastError();
}

hipError_t launch_select_lists(const uint64_t *keys, const Payload *pay, uint32_t nq, uint32_t m_stride, const uint32_t *m_dev,
                               uint32_t k, void *out, uint32_t out_stride, hipStream_t s, bool spread) {
  if (k == 0 || k > (uint32_t)kMaxFusedK || nq == 0 || nq > 65535 || !m_dev || out_stride < 16 + k * sizeof(Entry) || out_stride % 16)
    return hipErrorInvalidValue;
  const size_t lds = ((size_t)k + kSelCand) * 12;
  hipError_t e = allow_lds(select_topk_kernel, lds);
  if (e != hipSuccess) return e;
  // `spread` (lists of several hundred to a few thousand keys, a funnel group's): lists of up to kSpreadKeys keys go to
  // select_lists_spread_kernel, sixteen blocks each; the one-block kernel beside it takes the longer ones only
  const uint32_t skip = spread && m_stride > 1024 ? kSpreadKeys : 0u;
  if (skip)
    hipLaunchKernelGGL(select_lists_spread_kernel, dim3(kSpreadBlocks, nq), dim3(kSpreadThreads), 0, s, keys, pay, m_stride, m_dev, k,
                       static_cast<ResultBlock *>(out), out_stride);
  // (grid.y >= 2 is what makes the kernel index its lists by query: a batch of one goes through launch_select)
  hipLaunchKernelGGL(select_topk_kernel, dim3(1, nq), dim3(1024), lds, s, keys, pay, m_stride, k, 0ull, 0, nullptr,
                     static_cast<ResultBlock *>(out), 0u, nullptr, nullptr, m_dev, out_stride, skip);
  return hipGetLastError();
}

namespace {

// All of a short list (<= kSelListMax keys) in ascending key order, kEmptyKey entries dropped:
// the winners of a limit above kMaxFusedK leave the device in one launch.  One block, keys in
// LDS, rank sort (m^2 / 1024 compares per thread: ~55 us at m = 4096).
__global__ __launch_bounds__(1024) void sort_list_kernel(const uint64_t *__restrict__ keys, const Payload *__restrict__ pay,
                                                         uint32_t m, int *dev_status, BigResultHeader *head,
                                                         Entry *__restrict__ out) {
  extern __shared__ __align__(16) unsigned char sl_smem[];
  uint64_t *sk = reinterpret_cast<uint64_t *>(sl_smem);
  __shared__ uint32_t s_live;
  if (threadIdx.x == 0) s_live = 0;
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) sk[i] = keys[i];
  __syncthreads();
  uint32_t live = 0;
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
    const uint64_t ki = sk[i];
    if (ki == kEmptyKey) continue;
    live += 1;
    uint32_t pos = 0;
    for (uint32_t x = 0; x < m; ++x) {
      const uint64_t kx = sk[x];
      pos += (kx < ki || (kx == ki && x < i)) ? 1u : 0u;
    }
    const Payload p = pay[i];
    Entry e;
    e.key = ki;
    e.row = p.row;
    e.raw = p.raw;
    out[pos] = e;
  }
  atomicAdd(&s_live, live);
  __syncthreads();
  if (threadIdx.x == 0) {
    head->count = s_live;
    head->status = *dev_status;
    *dev_status = 0;
  }
}

}  // namespace

hipError_t launch_sort_list(const uint64_t *keys, const Payload *pay, uint32_t m, int *dev_status, BigResultHeader *head,
                            Entry *out, hipStream_t s) {
  if (m == 0 || m > kSelListMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sort_list_kernel, dim3(1), dim3(1024), (size_t)m * 8, s, keys, pay, m, dev_status, head, out);
  return hipGetLastError();
}

namespace {

// Cross-shard merge: world * k candidate entries (already sorted per shard) ->
// the k best overall by rank sort in LDS.  Keys are comparable across shards
// because every shard's id_rank column was taken from ONE ordering of all ids.
__global__ __launch_bounds__(256) void merge_blocks_kernel(const unsigned char *__restrict__ blocks, uint32_t world,
                                                           uint32_t k, uint32_t block_bytes, ResultBlock *out,
                                                           uint32_t *__restrict__ out_shard) {
  extern __shared__ __align__(16) unsigned char mb_smem[];
  uint64_t *keys = reinterpret_cast<uint64_t *>(mb_smem);  // [world * k]
  const uint32_t m = world * k;
  __shared__ uint32_t s_total;
  __shared__ int s_status;
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    int status = 0;
    for (uint32_t w = 0; w < world; ++w) {
      const ResultBlock *b = reinterpret_cast<const ResultBlock *>(blocks + (size_t)w * block_bytes);
      total += b->count < k ? b->count : k;
      status = b->status > status ? b->status : status;
    }
    s_total = total;
    s_status = status;
  }
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
    const uint32_t w = i / k, j = i - w * k;
    const ResultBlock *b = reinterpret_cast<const ResultBlock *>(blocks + (size_t)w * block_bytes);
    keys[i] = j < b->count ? b->e[j].key : kEmptyKey;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
    const uint64_t ki = keys[i];
    if (ki == kEmptyKey) continue;
    uint32_t pos = 0;
    for (uint32_t x = 0; x < m; ++x) {
      const uint64_t kx = keys[x];
      pos += (kx < ki || (kx == ki && x < i)) ? 1u : 0u;
    }
    if (pos < k) {
      const uint32_t w = i / k, j = i - w * k;
      const ResultBlock *b = reinterpret_cast<const ResultBlock *>(blocks + (size_t)w * block_bytes);
      out->e[pos] = b->e[j];
      out_shard[pos] = w;
    }
  }
  if (threadIdx.x == 0) {
    out->count = s_total < k ? s_total : k;
    out->status = s_status;
  }
}

}  // namespace

hipError_t launch_merge_blocks(const void *blocks, uint32_t world, uint32_t k, uint32_t block_bytes, ResultBlock *out,
                               uint32_t *out_shard, hipStream_t s) {
  if (world == 0 || k == 0 || k > (uint32_t)kMaxFusedK || (size_t)world * k * 8 > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(merge_blocks_kernel, dim3(1), dim3(256), (size_t)world * k * 8, s,
                     static_cast<const unsigned char *>(blocks), world, k, block_bytes, out, out_shard);
  return hipGetLastError();
}

namespace {

// ---------------------------------------------------------------------------
// Exact k-th smallest of a key column (limits above kMaxFusedK), no host decisions:
// three passes histogram 11-bit digits of the top 33 key bits among the keys that
// match the prefix resolved so far; every block re-derives that prefix from the
// previous passes' histograms (2 048 bins each), so a pass is one launch.  The
// collect pass appends the keys below the final prefix and those sharing it.
// ---------------------------------------------------------------------------
struct RadixPrefix {
  uint64_t prefix, mask;
  uint32_t krem;
};

// Digit q of a key: eleven bits from the top down, the sixth and last one the nine that remain
// (q = 0..2 cover the rank and the top id-rank bit, q = 3..5 the rest of the id rank).
__device__ __forceinline__ int radix_shift(int q) { return q < 5 ? 53 - 11 * q : 0; }
__device__ __forceinline__ uint32_t radix_digit_mask(int q) { return q < 5 ? kRadixBins - 1 : 511u; }

// Bin of `hist` holding the krem-th smallest (1-based), by one wave; updates krem.
__device__ __forceinline__ uint32_t radix_find_bin(const uint32_t *hist, uint32_t *krem, int lane, uint32_t last_bin) {
  constexpr uint32_t B = kRadixBins / kWave;  // bins per lane
  uint32_t mine = 0;
  for (uint32_t j = 0; j < B; ++j) mine += hist[lane * B + j];
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  const uint32_t excl = incl - mine;
  const uint32_t k = *krem;
  uint32_t bin = 0xFFFFFFFFu, below = 0;
  if (excl < k && k <= incl) {
    uint32_t cum = excl, b = lane * B;
    for (;; ++b) {
      if (cum + hist[b] >= k) break;
      cum += hist[b];
    }
    bin = b;
    below = cum;
  }
  // exactly one lane found it (or none when fewer than k keys exist: take the last bin)
  const uint64_t m = __ballot(bin != 0xFFFFFFFFu);
  const int src = m ? __ffsll((long long)m) - 1 : 0;
  const uint32_t rbin = __shfl(bin, src, kWave), rbelow = __shfl(below, src, kWave);
  if (!m) return last_bin;
  *krem = k - rbelow;
  return rbin;
}

// Prefix after `passes` resolved digits (wave 0 computes, everyone reads from LDS).
__device__ __forceinline__ RadixPrefix radix_prefix(const RadixArgs &a, int passes, uint32_t *lds_hist, RadixPrefix *s_out) {
  const int lane = threadIdx.x & (kWave - 1);
  RadixPrefix p;
  p.prefix = 0;
  p.mask = 0;
  p.krem = a.k;
  for (int q = 0; q < passes; ++q) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kRadixBins; i += blockDim.x) lds_hist[i] = a.hist[q * kRadixBins + i];
    __syncthreads();
    if (threadIdx.x < kWave) {
      uint32_t krem = p.krem;
      const uint32_t bin = radix_find_bin(lds_hist, &krem, lane, radix_digit_mask(q));
      const int shift = radix_shift(q);
      p.prefix |= (uint64_t)bin << shift;
      p.mask |= (uint64_t)radix_digit_mask(q) << shift;
      p.krem = krem;
      if (threadIdx.x == 0) *s_out = p;
    }
    __syncthreads();
    p = *s_out;
  }
  return p;
}

__global__ __launch_bounds__(256) void radix_pass_kernel(const RadixArgs a, int pass) {
  __shared__ uint32_t lds_hist[kRadixBins];
  __shared__ RadixPrefix s_p;
  if (pass == 0 && blockIdx.x == 0 && threadIdx.x == 0) *a.list_count = 0;
  const RadixPrefix p = radix_prefix(a, pass, lds_hist, &s_p);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kRadixBins; i += blockDim.x) lds_hist[i] = 0;
  __syncthreads();
  const int shift = radix_shift(pass);
  const uint32_t dmask = radix_digit_mask(pass);
  const u64x2 *k2 = reinterpret_cast<const u64x2 *>(a.keys);
  const uint32_t n2 = a.n / 2;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += gridDim.x * blockDim.x) {
    const u64x2 v = k2[i];
    if ((v.x & p.mask) == p.prefix) atomicAdd(&lds_hist[(uint32_t)(v.x >> shift) & dmask], 1u);
    if ((v.y & p.mask) == p.prefix) atomicAdd(&lds_hist[(uint32_t)(v.y >> shift) & dmask], 1u);
  }
  if ((a.n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t v = a.keys[a.n - 1];
    if ((v & p.mask) == p.prefix) atomicAdd(&lds_hist[(uint32_t)(v >> shift) & dmask], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kRadixBins; i += blockDim.x) {
    const uint32_t c = lds_hist[i];
    if (c) atomicAdd(&a.hist[pass * kRadixBins + i], c);
  }
}

__global__ __launch_bounds__(256) void radix_collect_kernel(const RadixArgs a) {
  __shared__ uint32_t lds_hist[kRadixBins];
  __shared__ RadixPrefix s_p;
  const RadixPrefix p = radix_prefix(a, a.passes == 6 ? 6 : 3, lds_hist, &s_p);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const uint64_t v = a.keys[i];
    if (v != kEmptyKey && (v & p.mask) <= p.prefix) {
      const uint32_t pos = atomicAdd(a.list_count, 1u);
      if (pos < a.cap) {
        a.list_keys[pos] = v;
        Payload pv;
        pv.row = i;
        pv.raw = a.pay_col ? a.pay_col[i].raw : 0.0f;  // (limits above kSelListMax: the list leaves the device as it is)
        a.list_pay[pos] = pv;
      } else {
        atomicMax(a.status, kStatusRetry);
      }
    }
  }
}

}  // namespace

hipError_t launch_radix_pass(const RadixArgs &a, int pass, uint32_t blocks, hipStream_t s) {
  if (pass < 0 || pass >= (a.passes == 6 ? 6 : 3) || a.n == 0 || a.k == 0 || ((uintptr_t)a.keys & 15)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(radix_pass_kernel, dim3(blocks), dim3(256), 0, s, a, pass);
  return hipGetLastError();
}

hipError_t launch_radix_collect(const RadixArgs &a, uint32_t blocks, hipStream_t s) {
  hipLaunchKernelGGL(radix_collect_kernel, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace vt

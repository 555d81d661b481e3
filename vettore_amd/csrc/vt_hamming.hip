// vt_hamming.hip -- the kernels over the packed bit matrix (gfx950): K4 Hamming scan + fused top-k, K4p pattern
// top-k for eight queries a sweep, K4h distance column + histogram + threshold collect, for one query and for
// eight.  Each kernel is followed by its LDS formula and its launcher.
#include "vt_scan.cuh"

#include <type_traits>
#include <utility>

namespace vt {

using namespace dev;

namespace {

// The row widths, in pairs of 64-bit words, that every templated kernel below is also built completely unrolled for
// (PAIRS > 0).  for_pairs calls f(std::integral_constant<int, P>{}) for the P that equals `pairs`; false when the width
// has no build of its own.
template <int... P, class F>
bool for_pairs_of(std::integer_sequence<int, P...>, uint32_t pairs, F &&f) {
  return ((pairs == (uint32_t)P && (f(std::integral_constant<int, P>{}), true)) || ...);
}
template <class F>
bool for_pairs(uint32_t pairs, F &&f) {
  return for_pairs_of(std::integer_sequence<int, 1, 2, 3, 4, 6, 8, 12, 16>{}, pairs, f);
}

// ---------------------------------------------------------------------------
// K4: packed sign-bit Hamming scan + fused top-k.  Replaces binary_top_k
// (search.rs:76-92) + packed_hamming (distances.rs:426-437, word_mask :472-481).
//
// The bit matrix is the index's own derived structure, so it is stored the way
// a wave wants to read it: per tile of 64 rows, word pair j of all 64 rows is
// contiguous ([tile][pair][row][2] u64).  Lane r then reads row r's words with
// fully coalesced 16-B loads (1 KiB per wave instruction) and owns the row's
// whole popcount: no cross-lane step, no LDS.  The query words are wave-uniform
// (scalar loads, SGPR operands).  PAIRS > 0 unrolls the row completely so every
// load of a tile is in flight before the first popcount.
// ---------------------------------------------------------------------------
template <int CAP, int PAIRS>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void hamming_topk_kernel(const HammingArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t pairs = PAIRS > 0 ? (uint32_t)PAIRS : a.pairs;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave_global = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t ntiles = (a.n + kWave - 1) / kWave;
  const uint32_t last_word = a.words - 1;
  const uint32_t rem = a.d % 64;
  const uint64_t last_mask = rem ? ((1ull << rem) - 1) : ~0ull;  // distances.rs:472-481 word_mask
  const u64x2 *bits = reinterpret_cast<const u64x2 *>(a.bits);
  extern __shared__ __align__(16) unsigned char hsmem[];

  WaveTopK<CAP> tk;
  tk.init(hsmem + wib * WaveTopK<CAP>::lds_bytes(), a.k);
  // Unrolled builds: the query's words (the host hands over an even count, the odd one out zero)
  // are read once, through the constant address space (s_load), and stay in SGPRs; only the last
  // word pair can hold the word that needs distances.rs:472-481's mask (words is 2 PAIRS - 1 or
  // 2 PAIRS), and a pad word is zero on both sides.
  typedef const __attribute__((address_space(4))) uint64_t *cu64_p;
  uint64_t qw[PAIRS > 0 ? 2 * PAIRS : 1];
  if (PAIRS > 0) {
#pragma unroll
    for (int j = 0; j < 2 * PAIRS; ++j) qw[j] = ((cu64_p)(uintptr_t)a.qbits)[j];
  }
  const uint64_t mask_even = a.words == 2u * PAIRS - 1 ? last_mask : ~0ull;
  // (an odd word count: the last pair's second word is a zero pad on both sides for whole rows, and the first word
  // BEHIND a prefix -- which must not count -- for a prefix pass)
  const uint64_t mask_odd = a.words == 2u * PAIRS ? last_mask : 0ull;
  const uint32_t tile_pairs = a.tile_pairs ? a.tile_pairs : pairs;
  for (uint32_t t = wave_global; t < ntiles; t += total_waves) {
    const u64x2 *base = bits + ((size_t)t * tile_pairs * kWave + lane);
    // `ham` counts the differing bits; in the pattern mode for jaccard `both` counts the bits set on
    // both sides as well
    uint32_t ham = 0, both = 0;
    if (PAIRS > 0) {
      u64x2 v[PAIRS > 0 ? PAIRS : 1];
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) v[j] = __builtin_nontemporal_load(base + (size_t)j * kWave);
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) {
        const uint64_t q0 = qw[2 * j], q1 = qw[2 * j + 1];
        if (j < PAIRS - 1) {
          ham += __popcll(v[j].x ^ q0) + __popcll(v[j].y ^ q1);
          if (a.jaccard) both += __popcll(v[j].x & q0) + __popcll(v[j].y & q1);
        } else {
          ham += __popcll((v[j].x ^ q0) & mask_even) + __popcll((v[j].y ^ q1) & mask_odd);
          if (a.jaccard) both += __popcll(v[j].x & q0 & mask_even) + __popcll(v[j].y & q1 & mask_odd);
        }
      }
    } else {
      for (uint32_t j = 0; j < pairs; ++j) {
        const u64x2 v = __builtin_nontemporal_load(base + (size_t)j * kWave);
        const uint32_t w0 = 2 * j, w1 = 2 * j + 1;
        const uint64_t q0 = a.qbits[w0], q1 = w1 < a.words ? a.qbits[w1] : 0ull;
        const uint64_t m0 = w0 == last_word ? last_mask : ~0ull, m1 = w1 < a.words ? (w1 == last_word ? last_mask : ~0ull) : 0ull;
        ham += __popcll((v.x ^ q0) & m0) + __popcll((v.y ^ q1) & m1);
        if (a.jaccard) both += __popcll(v.x & q0 & m0) + __popcll(v.y & q1 & m1);
      }
    }
    const uint32_t grow = t * kWave + lane;
    bool valid = grow < a.n;
    const uint32_t my_rank = (valid && a.id_rank) ? a.id_rank[grow] : grow;
    float raw = (float)ham;  // distance as f32 (distances.rs:436; :319-324 over non-zero bits)
    if (a.jaccard) {         // distances.rs:327-347: union = differing + common coordinates
      const uint32_t uni = ham + both;
      raw = uni == 0 ? 0.0f : 1.0f - (float)both / (float)uni;
    }
    const uint64_t key = ((uint64_t)orderable(raw) << 32) | my_rank;
    if (a.has_lo) valid = valid && key > a.lo_key;
    tk.offer(valid, key, grow, raw, lane);
  }
  __shared__ uint32_t s_counts[kWavesPerBlock];
  tk.merge_block(wib, kWavesPerBlock, s_counts, lane);
  if (wib == 0) tk.store(a.part_keys + (size_t)blockIdx.x * a.k, a.part_pay + (size_t)blockIdx.x * a.k, lane);
}

template <int CAP>
hipError_t launch_hamming_r(const HammingArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = kWavesPerBlock * WaveTopK<CAP>::lds_bytes();
  const dim3 grid(blocks), block(kWavesPerBlock * kWave);
  if (!for_pairs(a.pairs, [&](auto P) { hipLaunchKernelGGL((hamming_topk_kernel<CAP, P.value>), grid, block, lds, s, a); }))
    hipLaunchKernelGGL((hamming_topk_kernel<CAP, 0>), grid, block, lds, s, a);
  return hipGetLastError();
}

}  // namespace

size_t hamming_lds_bytes(uint32_t k) {
  return kWavesPerBlock * (k <= (uint32_t)kSmallK ? WaveTopK<kCapSmall>::lds_bytes() : WaveTopK<kCapLarge>::lds_bytes());
}

hipError_t launch_hamming(const HammingArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.k == 0 || a.k > (uint32_t)kMaxFusedK || a.words == 0 || a.pairs != (a.words + 1) / 2 || (a.tile_pairs && a.tile_pairs < a.pairs))
    return hipErrorInvalidValue;
  return a.k <= (uint32_t)kSmallK ? launch_hamming_r<kCapSmall>(a, blocks, s) : launch_hamming_r<kCapLarge>(a, blocks, s);
}

namespace {

// ---------------------------------------------------------------------------
// K4p: flat_search under float hamming / jaccard for up to kPatternMultiMax queries in ONE sweep
// of the non-zero-bit column (batches; callers that met on a handle).  A lane owns a row as in
// K4 and keeps its words in registers; the queries' words are wave-uniform (scalar loads), so a
// query costs the popcounts and one offer to ITS wave list -- the tile is read once.  Scores and
// keys as in K4's pattern mode (distances.rs:319-347); lists of k <= kSmallK per (query, wave),
// merged per block and filed per query for launch_select_queries.  Padding bits are zero on both
// sides (K5 and the host's query packing write none), so no word needs a mask.
// ---------------------------------------------------------------------------
template <int PAIRS, bool JACCARD>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void pattern_topk_multi_kernel(const PatternMultiArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave_global = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t ntiles = (a.n + kWave - 1) / kWave;
  const u64x2 *bits = reinterpret_cast<const u64x2 *>(a.bits);
  extern __shared__ __align__(16) unsigned char hsmem[];
  constexpr size_t kList = WaveTopK<kCapSmall>::lds_bytes();
  uint32_t *s_counts = reinterpret_cast<uint32_t *>(hsmem + (size_t)kPatternMultiMax * kWavesPerBlock * kList);

  WaveTopK<kCapSmall> tk[kPatternMultiMax];
#pragma unroll
  for (int q = 0; q < (int)kPatternMultiMax; ++q) tk[q].init(hsmem + ((size_t)q * kWavesPerBlock + wib) * kList, a.k);
  // 64 KB of lists leave two blocks on a CU -- two waves per SIMD, too few to hide a trip to HBM
  // behind the other wave's popcounts -- so a wave keeps its next U tiles in flight while it works
  // on the current U (registers are what this kernel has to spare).
  // A query's words are scalar loads: their latency is paid once per query and U tiles, not per tile.
  constexpr int U = PAIRS <= 4 ? 4 : PAIRS <= 6 ? 3 : PAIRS <= 8 ? 2 : 1;
  u64x2 cur[U][PAIRS], nxt[U][PAIRS];
  auto load_tiles = [&](u64x2(&dst)[U][PAIRS], uint32_t t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t t = t0 + (uint32_t)u * total_waves;
      if (t < ntiles) {
        const u64x2 *base = bits + ((size_t)t * PAIRS * kWave + lane);
#pragma unroll
        for (int j = 0; j < PAIRS; ++j) dst[u][j] = __builtin_nontemporal_load(base + (size_t)j * kWave);
      }
    }
  };
  load_tiles(cur, wave_global);
  for (uint32_t t0 = wave_global; t0 < ntiles; t0 += (uint32_t)U * total_waves) {
    // (the id ranks of the CURRENT tiles are asked for before the next tiles' words: loads return in order, so a rank
    // requested behind the prefetch could only be waited for together with it -- every iteration then drained what it
    // had just put in flight)
    uint32_t grow[U], my_rank[U];
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t t = t0 + (uint32_t)u * total_waves;
      grow[u] = t * kWave + lane;
      valid[u] = t < ntiles && grow[u] < a.n;
      my_rank[u] = (valid[u] && a.id_rank) ? a.id_rank[grow[u]] : grow[u];
    }
    load_tiles(nxt, t0 + (uint32_t)U * total_waves);
    // jaccard: |x or q| = |x| + |q| - |x and q|, and |x| is the row's own (once per tile, not per
    // query), |q| a scalar: a query costs one v_and + one v_bcnt per 32 row bits, like hamming's xor
    uint32_t px[U];
    if (JACCARD) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        px[u] = 0;
#pragma unroll
        for (int j = 0; j < PAIRS; ++j) px[u] += __popcll(cur[u][j].x) + __popcll(cur[u][j].y);
      }
    }
#pragma unroll
    for (int q = 0; q < (int)kPatternMultiMax; ++q) {
      if ((uint32_t)q < a.nq) {  // (wave-uniform)
        // (read through the constant address space => s_load, and the words enter v_xor / v_and as
        // SGPR operands, as in K4hm: nothing writes them while the kernel runs)
        typedef const __attribute__((address_space(4))) uint64_t *cu64_p;
        const cu64_p qb = (cu64_p)(uintptr_t)a.qbits + (size_t)q * 2 * PAIRS;
        uint64_t qw[2 * PAIRS];
#pragma unroll
        for (int j = 0; j < 2 * PAIRS; ++j) qw[j] = qb[j];
        uint32_t pq = 0;
        if (JACCARD) {
#pragma unroll
          for (int j = 0; j < 2 * PAIRS; ++j) pq += __popcll(qw[j]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (t0 + (uint32_t)u * total_waves < ntiles) {  // (wave-uniform)
            uint32_t ham = 0, both = 0;
#pragma unroll
            for (int j = 0; j < PAIRS; ++j) {
              if (JACCARD) both += __popcll(cur[u][j].x & qw[2 * j]) + __popcll(cur[u][j].y & qw[2 * j + 1]);
              else ham += __popcll(cur[u][j].x ^ qw[2 * j]) + __popcll(cur[u][j].y ^ qw[2 * j + 1]);
            }
            float raw = (float)ham;
            if (JACCARD) {
              const uint32_t uni = px[u] + pq - both;
              raw = uni == 0 ? 0.0f : 1.0f - (float)both / (float)uni;
            }
            const uint64_t key = ((uint64_t)orderable(raw) << 32) | my_rank[u];
            tk[q].offer(valid[u], key, grow[u], raw, lane);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) cur[u][j] = nxt[u][j];
  }
#pragma unroll
  for (int q = 0; q < (int)kPatternMultiMax; ++q) {
    if ((uint32_t)q < a.nq) {
      tk[q].merge_block(wib, kWavesPerBlock, s_counts + q * kWavesPerBlock, lane);
      if (wib == 0) {
        const size_t list = ((size_t)(a.first_query + q) * gridDim.x + blockIdx.x) * a.k;
        tk[q].store(a.part_keys + list, a.part_pay + list, lane);
      }
    }
  }
}

}  // namespace

size_t pattern_multi_lds_bytes() {
  return (size_t)kPatternMultiMax * kWavesPerBlock * WaveTopK<kCapSmall>::lds_bytes() + kPatternMultiMax * kWavesPerBlock * sizeof(uint32_t);
}
bool pattern_multi_supports(uint32_t pairs) {
  return for_pairs(pairs, [](auto) {});
}
hipError_t launch_pattern_multi(const PatternMultiArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.k == 0 || a.k > (uint32_t)kSmallK || a.nq == 0 || a.nq > kPatternMultiMax || a.pairs != (a.words + 1) / 2 ||
      !pattern_multi_supports(a.pairs))
    return hipErrorInvalidValue;
  const size_t lds = pattern_multi_lds_bytes();
  hipError_t e = hipErrorInvalidValue;  // (no run-time-width build of this kernel)
  for_pairs(a.pairs, [&](auto P) {
    auto go = [&](auto kern) {
      e = allow_lds(kern, lds);
      if (e != hipSuccess) return;
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
      e = hipGetLastError();
    };
    if (a.jaccard) go(pattern_topk_multi_kernel<P.value, true>);
    else go(pattern_topk_multi_kernel<P.value, false>);
  });
  return e;
}

namespace {

// ---------------------------------------------------------------------------
// K4h: the Hamming candidate pass as a pure stream (resident corpus, k <= 256).
// Distances are integers 0..d, so the k-th smallest is found exactly from a
// histogram instead of carrying k-entry lists through the scan:
//   hamming_dist_kernel     popcounts as in K4; writes the 2-byte distance of every
//                           row and accumulates a (d+1)-bin histogram (LDS, flushed
//                           once per block);
//   hamming_collect_kernel  every block finds D* = the k-th smallest distance from
//                           the histogram, then the grid sweeps the distance column
//                           (2 bytes per row) and appends the rows with distance <=
//                           D* -- all winners plus the ties at D* -- to one list,
//                           keyed (distance, id rank); K3 selects the k best.
// The scan neither reads id ranks nor touches candidate buffers, so its time does
// not depend on k (K4: 168 us at k = 10, 249 us at k = 256 for 10M rows).
// Two histograms alternate between queries: the collect pass of one query clears
// the histogram of the next, block 0 of the distance pass clears the list counter.
// ---------------------------------------------------------------------------
template <int PAIRS>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void hamming_dist_kernel(const HammingHistArgs a) {
  extern __shared__ uint32_t hh_lds[];  // [d + 1]
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t pairs = PAIRS > 0 ? (uint32_t)PAIRS : a.pairs;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave_global = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t ntiles = (a.n + kWave - 1) / kWave;
  const uint32_t last_word = a.words - 1;
  const uint32_t rem = a.d % 64;
  const uint64_t last_mask = rem ? ((1ull << rem) - 1) : ~0ull;  // distances.rs:472-481 word_mask
  const u64x2 *bits = reinterpret_cast<const u64x2 *>(a.bits);
  for (uint32_t i = threadIdx.x; i <= a.d; i += blockDim.x) hh_lds[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.list_count = 0;
  __syncthreads();
  // (query words in SGPRs, a mask on the last word pair only: as in K4)
  typedef const __attribute__((address_space(4))) uint64_t *cu64_p;
  uint64_t qw[PAIRS > 0 ? 2 * PAIRS : 1];
  if (PAIRS > 0) {
#pragma unroll
    for (int j = 0; j < 2 * PAIRS; ++j) qw[j] = ((cu64_p)(uintptr_t)a.qbits)[j];
  }
  const uint64_t mask_even = a.words == 2u * PAIRS - 1 ? last_mask : ~0ull;
  const uint64_t mask_odd = a.words == 2u * PAIRS ? last_mask : ~0ull;
  for (uint32_t t = wave_global; t < ntiles; t += total_waves) {
    const u64x2 *base = bits + ((size_t)t * pairs * kWave + lane);
    uint32_t ham = 0;
    if (PAIRS > 0) {
      u64x2 v[PAIRS > 0 ? PAIRS : 1];
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) v[j] = __builtin_nontemporal_load(base + (size_t)j * kWave);
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) {
        const uint64_t q0 = qw[2 * j], q1 = qw[2 * j + 1];
        if (j < PAIRS - 1) ham += __popcll(v[j].x ^ q0) + __popcll(v[j].y ^ q1);
        else ham += __popcll((v[j].x ^ q0) & mask_even) + __popcll((v[j].y ^ q1) & mask_odd);
      }
    } else {
      for (uint32_t j = 0; j < pairs; ++j) {
        const u64x2 v = __builtin_nontemporal_load(base + (size_t)j * kWave);
        const uint32_t w0 = 2 * j, w1 = 2 * j + 1;
        const uint64_t q0 = a.qbits[w0], q1 = w1 < a.words ? a.qbits[w1] : 0ull;
        const uint64_t m0 = w0 == last_word ? last_mask : ~0ull, m1 = w1 == last_word ? last_mask : ~0ull;
        ham += __popcll((v.x ^ q0) & m0) + __popcll((v.y ^ q1) & m1);
      }
    }
    const uint32_t grow = t * kWave + lane;
    if (grow < a.n) {
      a.dist[grow] = (uint16_t)ham;
      atomicAdd(&hh_lds[ham], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i <= a.d; i += blockDim.x) {
    const uint32_t c = hh_lds[i];
    if (c) atomicAdd(&a.hist[i], c);
  }
}

}  // namespace

size_t hamming_hist_lds_bytes(uint32_t d) { return ((size_t)d + 1) * sizeof(uint32_t); }

hipError_t launch_hamming_dist(const HammingHistArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.words == 0 || a.pairs != (a.words + 1) / 2 || a.d > kHammingHistMaxDim) return hipErrorInvalidValue;
  const size_t lds = hamming_hist_lds_bytes(a.d);
  const dim3 grid(blocks), block(kWavesPerBlock * kWave);
  if (!for_pairs(a.pairs, [&](auto P) { hipLaunchKernelGGL((hamming_dist_kernel<P.value>), grid, block, lds, s, a); }))
    hipLaunchKernelGGL((hamming_dist_kernel<0>), grid, block, lds, s, a);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(256) void hamming_collect_kernel(const HammingCollectArgs a0) {
  extern __shared__ uint32_t hc_lds[];  // [d + 1]
  __shared__ uint32_t s_dstar;
  const HammingCollectArgs &a = a0;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t bins = a.d + 1;
  for (uint32_t i = threadIdx.x; i < bins; i += blockDim.x) hc_lds[i] = a.hist[i];
  // clear the other histogram for the next query (grid-wide, bins are few)
  if (a.hist_next)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < bins; i += gridDim.x * blockDim.x) a.hist_next[i] = 0;
  __syncthreads();
  if (threadIdx.x < kWave) {
    // D* = smallest D with count(distance <= D) >= k; lane l owns bins [l*B, (l+1)*B)
    const uint32_t B = (bins + kWave - 1) / kWave;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < B; ++j) {
      const uint32_t b = lane * B + j;
      mine += b < bins ? hc_lds[b] : 0u;
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t t = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += t;
    }
    const uint32_t excl = incl - mine;
    const uint32_t total = __shfl(incl, kWave - 1, kWave);
    if (lane == 0 && total < a.k) s_dstar = a.d;  // fewer rows than k: everything qualifies
    if (excl < a.k && a.k <= incl) {
      uint32_t cum = excl, b = lane * B;
      for (;; ++b) {
        cum += hc_lds[b];
        if (cum >= a.k) break;
      }
      s_dstar = b;
    }
  }
  __syncthreads();
  const uint32_t dstar = s_dstar;
  // sweep the distance column, 8 rows (16 bytes) per load
  const uint32_t n8 = (a.n + 7) / 8;
  const u64x2 *d8 = reinterpret_cast<const u64x2 *>(a.dist);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += gridDim.x * blockDim.x) {
    const u64x2 v = d8[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t row = i * 8 + j;
      const uint32_t dv = (uint32_t)(((j < 4 ? v.x : v.y) >> (16 * (j & 3))) & 0xFFFFu);
      if (row < a.n && dv <= dstar) {
        const uint32_t pos = atomicAdd(a.list_count, 1u);
        if (pos < a.cap) {
          const float raw = (float)dv;  // distance as f32 (distances.rs:436)
          const uint32_t rk = a.id_rank ? a.id_rank[row] : row;
          a.keys[pos] = ((uint64_t)orderable(raw) << 32) | rk;
          Payload p;
          p.row = row;
          p.raw = raw;
          a.pay[pos] = p;
        } else {
          atomicMax(a.status, kStatusRetry);  // more ties than the list holds: the caller takes the K4 path
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_hamming_collect(const HammingCollectArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.d > kHammingHistMaxDim || a.k == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hamming_collect_kernel, dim3(blocks), dim3(256), hamming_hist_lds_bytes(a.d), s, a);
  return hipGetLastError();
}

namespace {

// K4h's distance pass for up to kHammingMultiMax (8) queries at once: the bit tiles are read
// ONCE, every lane popcounts its row against all the queries, writes the eight 2-byte distances
// of its row as one 16-byte store (dist[row][8]) and counts them in nq LDS histograms.
// Concurrent quantized_search callers (collection.ex:276-295 under the read lock) then share a
// sweep of the 0.96-GB bit matrix the way plain searches share a scan of the rows.
// The query words are wave-uniform: they come through the scalar cache (constant address space
// => s_load) and enter v_xor as SGPR operands -- with the words in LDS (a ds_read_b64 per word
// and query, then moves) eight queries were VALU-bound at 1.45x the single pass; this is two
// vector instructions per 32 row bits and query.
template <int PAIRS>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void hamming_dist_multi_kernel(const HammingMultiArgs a) {
  extern __shared__ __align__(16) uint32_t hm_lds[];  // [nq][d + 1] histograms
  typedef const __attribute__((address_space(4))) uint64_t *cu64_p;
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t pairs = PAIRS > 0 ? (uint32_t)PAIRS : a.pairs;
  const uint32_t bins = a.d + 1;
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave_global = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t ntiles = (a.n + kWave - 1) / kWave;
  const uint32_t rem = a.d % 64;
  const uint64_t last_mask = rem ? ((1ull << rem) - 1) : ~0ull;  // distances.rs:472-481 word_mask
  for (uint32_t i = threadIdx.x; i < a.nq * bins; i += blockDim.x) hm_lds[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < kHammingMultiMax) a.list_count[threadIdx.x] = 0;
  __syncthreads();
  // (the host packs the queries' words with their padding bits clear and an even word count:
  // qbits[q][2 * pairs])
  cu64_p qc = (cu64_p)(uintptr_t)a.qbits;
  const u64x2 *bits = reinterpret_cast<const u64x2 *>(a.bits);
  for (uint32_t t = wave_global; t < ntiles; t += total_waves) {
    const u64x2 *base = bits + ((size_t)t * pairs * kWave + lane);
    const uint32_t grow = t * kWave + lane;
    auto row_words = [&](uint32_t j) -> u64x2 {
      u64x2 v = __builtin_nontemporal_load(base + (size_t)j * kWave);
      // (packed_hamming masks both operands' last word; the matrix's own padding is zero already)
      if (2 * j == a.words - 1) v.x &= last_mask;
      if (2 * j + 1 == a.words - 1) v.y &= last_mask;
      if (2 * j + 1 >= a.words) v.y = 0ull;
      return v;
    };
    // All eight query slots are computed (the host zero-fills the unused ones): no branches in
    // here.  The words of a query are fetched anew for every tile -- hoisted out of the tile loop
    // they are 192 SGPRs, which the compiler then parks in vector lanes (v_writelane / v_readlane
    // around every use: the pass was VALU-bound at 1.45x the single one).
    uint32_t ham[kHammingMultiMax];
    typedef const __attribute__((address_space(4))) uint32_t *cu32_p;
    if (PAIRS > 0) {
      // (no masking of the last word here: the matrix's padding bits and pad word are zero by
      // construction -- sign_pack writes bits j < d only, into zeroed words -- and so are the query's,
      // so they contribute nothing to the xor; the masks were 36 of ~600 vector instructions per tile)
      u64x2 v[PAIRS > 0 ? PAIRS : 1];
#pragma unroll
      for (int j = 0; j < PAIRS; ++j) v[j] = __builtin_nontemporal_load(base + (size_t)j * kWave);
#pragma unroll
      for (uint32_t q = 0; q < kHammingMultiMax; ++q) {
        uint64_t qaddr = (uint64_t)(uintptr_t)a.qbits + (uint64_t)q * 2 * PAIRS * 8;
        asm volatile("" : "+s"(qaddr));  // (not loop-invariant as far as the compiler can tell)
        cu32_p w = (cu32_p)(uintptr_t)qaddr;
        uint32_t h = 0;
#pragma unroll
        for (int j = 0; j < PAIRS; ++j) {
          h = __builtin_popcount((uint32_t)v[j].x ^ w[4 * j]) + h;
          h = __builtin_popcount((uint32_t)(v[j].x >> 32) ^ w[4 * j + 1]) + h;
          h = __builtin_popcount((uint32_t)v[j].y ^ w[4 * j + 2]) + h;
          h = __builtin_popcount((uint32_t)(v[j].y >> 32) ^ w[4 * j + 3]) + h;
        }
        ham[q] = h;
      }
    } else {
#pragma unroll
      for (uint32_t q = 0; q < kHammingMultiMax; ++q) ham[q] = 0;
      for (uint32_t j = 0; j < pairs; ++j) {
        const u64x2 v = row_words(j);
#pragma unroll
        for (uint32_t q = 0; q < kHammingMultiMax; ++q) {
          cu64_p w = qc + (size_t)q * 2 * pairs;
          ham[q] += __popcll(v.x ^ w[2 * j]) + __popcll(v.y ^ w[2 * j + 1]);
        }
      }
    }
    if (grow < a.n) {
      uint32_t packed[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) packed[i] = ham[2 * i] | (ham[2 * i + 1] << 16);
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      reinterpret_cast<u32x4 *>(a.dist)[grow] = u32x4{packed[0], packed[1], packed[2], packed[3]};
#pragma unroll
      for (uint32_t q = 0; q < kHammingMultiMax; ++q)
        if (q < a.nq) atomicAdd(&hm_lds[q * bins + ham[q]], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.nq * bins; i += blockDim.x) {
    const uint32_t c = hm_lds[i];
    if (c) {
      const uint32_t q = i / bins;
      atomicAdd(&a.hist[(size_t)q * a.hist_stride + (i - q * bins)], c);
    }
  }
}

}  // namespace

size_t hamming_multi_lds_bytes(uint32_t d, uint32_t words, uint32_t nq) {
  (void)words;
  return (size_t)nq * (d + 1) * sizeof(uint32_t);
}

hipError_t launch_hamming_dist_multi(const HammingMultiArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.words == 0 || a.pairs != (a.words + 1) / 2 || a.nq == 0 || a.nq > kHammingMultiMax || a.hist_stride < a.d + 1 ||
      ((uintptr_t)a.dist & 15) || ((uintptr_t)a.qbits & 15))
    return hipErrorInvalidValue;
  const size_t lds = hamming_multi_lds_bytes(a.d, a.words, a.nq);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  const dim3 grid(blocks), block(kWavesPerBlock * kWave);
  if (!for_pairs(a.pairs, [&](auto P) { hipLaunchKernelGGL((hamming_dist_multi_kernel<P.value>), grid, block, lds, s, a); }))
    hipLaunchKernelGGL((hamming_dist_multi_kernel<0>), grid, block, lds, s, a);
  return hipGetLastError();
}

namespace {

// The collect pass for the nq queries of a group in ONE sweep of the interleaved distance column
// (16 bytes per row): every block finds the nq thresholds D*_q from the nq histograms, then each
// lane takes a row's eight distances and appends the row to the list of every query it
// qualifies for (keyed (distance, id rank), as hamming_collect_kernel does for one).
__global__ __launch_bounds__(256) void hamming_collect_multi_kernel(const HammingCollectArgs a, uint32_t nq) {
  extern __shared__ uint32_t hcm_lds[];  // [d + 1] one histogram at a time
  __shared__ uint32_t s_dstar[kHammingMultiMax];
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t bins = a.d + 1;
  for (uint32_t q = 0; q < nq; ++q) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < bins; i += blockDim.x) hcm_lds[i] = a.hist[(size_t)q * a.hist_stride + i];
    __syncthreads();
    if (threadIdx.x < kWave) {
      // D* = smallest D with count(distance <= D) >= k; lane l owns bins [l*B, (l+1)*B)
      const uint32_t B = (bins + kWave - 1) / kWave;
      uint32_t mine = 0;
      for (uint32_t j = 0; j < B; ++j) {
        const uint32_t b = lane * B + j;
        mine += b < bins ? hcm_lds[b] : 0u;
      }
      uint32_t incl = mine;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, kWave);
        if (lane >= o) incl += t;
      }
      const uint32_t excl = incl - mine;
      const uint32_t total = __shfl(incl, kWave - 1, kWave);
      if (lane == 0 && total < a.k) s_dstar[q] = a.d;  // fewer rows than k: everything qualifies
      if (excl < a.k && a.k <= incl) {
        uint32_t cum = excl, b = lane * B;
        for (;; ++b) {
          cum += hcm_lds[b];
          if (cum >= a.k) break;
        }
        s_dstar[q] = b;
      }
    }
  }
  __syncthreads();
  uint32_t dstar[kHammingMultiMax];
#pragma unroll
  for (uint32_t q = 0; q < kHammingMultiMax; ++q) dstar[q] = q < nq ? s_dstar[q] : 0u;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 *d4 = reinterpret_cast<const u32x4 *>(a.dist);
  for (uint32_t row = blockIdx.x * blockDim.x + threadIdx.x; row < a.n; row += gridDim.x * blockDim.x) {
    const u32x4 v = d4[row];
    uint32_t rk = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t q = 0; q < kHammingMultiMax; ++q) {
      const uint32_t dv = (v[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
      if (q < nq && dv <= dstar[q]) {
        if (rk == 0xFFFFFFFFu) rk = a.id_rank ? a.id_rank[row] : row;
        const uint32_t pos = atomicAdd(a.list_count + q, 1u);
        if (pos < a.cap) {
          const float raw = (float)dv;  // distance as f32 (distances.rs:436)
          a.keys[(size_t)q * a.cap + pos] = ((uint64_t)orderable(raw) << 32) | rk;
          Payload p;
          p.row = row;
          p.raw = raw;
          a.pay[(size_t)q * a.cap + pos] = p;
        } else {
          atomicMax(a.status, kStatusRetry);  // more ties than the list holds: the caller takes the queries one by one
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_hamming_collect_multi(const HammingCollectArgs &a, uint32_t blocks, uint32_t nq, hipStream_t s) {
  if (a.d > kHammingHistMaxDim || a.k == 0 || nq == 0 || nq > kHammingMultiMax || a.hist_next) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hamming_collect_multi_kernel, dim3(blocks), dim3(256), hamming_hist_lds_bytes(a.d), s, a, nq);
  return hipGetLastError();
}

}  // namespace vt

// vt_hnsw.hip -- K11: HNSW traversals on the device (gfx950): a whole `search` (hnsw.rs:292-333) or a whole insert's
// descent (hnsw.rs:179-207) per wave, many traversals per launch, no host round trip between hops.
//
// One block is one wave is one traversal.  A traversal is a program of the reference's greedy_closest (hnsw.rs:336-372)
// and search_layer (:375-434) over the device mirror of the graph (HnswDev: fixed-stride lists of slab rows -- rows are
// handed out in the order of the internal ids, so (distance, row) orders like the reference's (distance, internal id))
// and the slab of rows.
//
// Distances: rank_distance(metric, stored row, query) (distances.rs:108-119) is one lane's own serial chain in the
// reference's order -- vt_pair.cuh's f32 chain, stored row on the left, and its finish_raw with the recovery by value -- so a
// hop's neighbours are scored side by side, one lane each: the unvisited neighbours of up to 64 list entries are
// compacted into a pending list, their rows staged into the wave's LDS tile with coalesced 16-byte loads, `tt` rows at
// a time (tt = 64 down to 2 by the row length), and lane r walks row r of the tile against the query, which sits in
// LDS too.  Rows longer than kHnswLdsDim floats are walked where they lie, the query with them (STAGED = false).
// What the reference then does with the distances -- acceptance in list order against a `worst` read once per popped
// candidate, the two heaps, the IEEE `<` / `>` beside the total order -- is serial: lane 0 runs it over the pending
// list.  The heaps order by one u64 key, orderable(dist) << 32 | row: f32::total_cmp, then the id.
//
// Scratch, per traversal slot in global memory: a candidate heap and a result heap of `cap` keys each and an open
// hash of 2 * cap rows for the visited set (fresh per search_layer).  A traversal that would visit more than `cap`
// nodes, or whose ef exceeds it, ends with kHnswRetry and changes nothing the host uses: the host runs it again with
// cap >= nodes + 64, which no traversal outgrows.
//
// K11c, further down: the compaction of the slab and the mirror into fresh buffers once dead rows outnumber live ones
// (host/vt_hnswplan.h) -- a gather of rows and a renumbering of every list entry, nothing of the traversal's.
#include "vt_pair.cuh"

namespace vt {
namespace dev {

namespace {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;

__device__ __forceinline__ float key_dist(uint64_t key) {  // orderable()'s inverse
  return from_orderable((uint32_t)(key >> 32));
}
__device__ __forceinline__ uint64_t make_key(float dist, uint32_t row) { return ((uint64_t)orderable(dist) << 32) | row; }
__device__ __forceinline__ float rank_of(int metric, float raw) {  // distances.rs:113-119 rank_value
  if (metric == M_COS) return 1.0f - raw;
  if (metric == M_IP) return -raw;
  return raw;
}

// binary heaps over u64 keys in the slot's scratch, run by one lane
__device__ __forceinline__ void min_push(uint64_t *h, uint32_t &n, uint64_t k) {
  uint32_t i = n++;
  while (i > 0) {
    const uint32_t p = (i - 1) >> 1;
    const uint64_t hp = h[p];
    if (hp <= k) break;
    h[i] = hp;
    i = p;
  }
  h[i] = k;
}
__device__ __forceinline__ uint64_t min_pop(uint64_t *h, uint32_t &n) {
  const uint64_t top = h[0];
  const uint64_t last = h[--n];
  uint32_t i = 0;
  for (;;) {
    uint32_t c = 2 * i + 1;
    if (c >= n) break;
    uint64_t hc = h[c];
    if (c + 1 < n) {
      const uint64_t hr = h[c + 1];
      if (hr < hc) {
        hc = hr;
        ++c;
      }
    }
    if (hc >= last) break;
    h[i] = hc;
    i = c;
  }
  if (n) h[i] = last;
  return top;
}
__device__ __forceinline__ void max_push(uint64_t *h, uint32_t &n, uint64_t k) {
  uint32_t i = n++;
  while (i > 0) {
    const uint32_t p = (i - 1) >> 1;
    const uint64_t hp = h[p];
    if (hp >= k) break;
    h[i] = hp;
    i = p;
  }
  h[i] = k;
}
__device__ __forceinline__ void max_replace_top(uint64_t *h, uint32_t n, uint64_t k) {
  uint32_t i = 0;
  for (;;) {
    uint32_t c = 2 * i + 1;
    if (c >= n) break;
    uint64_t hc = h[c];
    if (c + 1 < n) {
      const uint64_t hr = h[c + 1];
      if (hr > hc) {
        hc = hr;
        ++c;
      }
    }
    if (hc <= k) break;
    h[i] = hc;
    i = c;
  }
  h[i] = k;
}

// One wave's traversal state: wave-uniform but for `lane`.
struct Trav {
  HnswDev g;
  int metric;
  uint32_t lane;
  const float *q;     // the query: LDS when staged, else global
  float *tile;        // [tt][ld]
  uint32_t tt, ld;
  uint32_t *pend;     // LDS [64]: the rows whose distances are wanted, in list order
  float *praw;        // LDS [64]: their raw values
  uint64_t *cand, *res;  // [cap] each
  uint32_t *visited;     // [2 * cap], kNoRow = free
  uint32_t cap, hshift;  // slot of a row: (row * 2654435761) >> hshift
};

// the list of `row` on `layer`: its length and entries (a node below the layer has none)
__device__ __forceinline__ const uint32_t *list_of(const HnswDev &g, uint32_t row, uint32_t layer, uint32_t *count) {
  const uint32_t *l;
  if (layer == 0) {
    l = g.adj0 + (size_t)row * (g.m0 + 1);
  } else {
    if (g.level[row] < layer) {
      *count = 0;
      return g.adj0;
    }
    l = g.upper + (size_t)g.upoff[row] + (size_t)(layer - 1) * (g.m + 1);
  }
  const uint32_t c = l[0];
  const uint32_t lim = layer == 0 ? g.m0 : g.m;
  *count = c < lim ? c : lim;
  return l + 1;
}

// praw[j] = compute(metric, row pend[j], query) for j < m <= 64; false: a pair failed ("metric overflow")
template <int OP, int ORDER, bool STAGED>
__device__ __forceinline__ bool eval_pending(const Trav &t, uint32_t m) {
  const uint32_t lane = t.lane, d = t.g.d;
  const uint32_t step = STAGED ? t.tt : (uint32_t)kWave;
  bool bad = false;
  wave_lds_fence();  // pend is written
  for (uint32_t j0 = 0; j0 < m; j0 += step) {
    const uint32_t cnt = m - j0 < step ? m - j0 : step;
    if (STAGED) {
      wave_lds_fence();  // the readers of the tile's previous rows are done
      const uint32_t rs4 = (uint32_t)t.g.stride / 4, ld4 = t.ld / 4;
      const uint32_t units = cnt * rs4;
      for (uint32_t u = lane; u < units; u += kWave) {
        const uint32_t r = u / rs4, c = u - r * rs4;
        const f32x4 *src = reinterpret_cast<const f32x4 *>(t.g.X + (size_t)t.pend[j0 + r] * t.g.stride);
        reinterpret_cast<f32x4 *>(t.tile)[r * ld4 + c] = src[c];
      }
      wave_lds_fence();
    }
    if (lane < cnt) {
      const float *x = STAGED ? t.tile + (size_t)lane * t.ld : t.g.X + (size_t)t.pend[j0 + lane] * t.g.stride;
      const float *const q[1] = {t.q};
      float raw[1];
      f32_raws<OP, ORDER, 1, true, false>(t.metric, q, x, d, raw);  // left = stored row, right = query
      t.praw[j0 + lane] = raw[0];
      bad = bad || raw[0] != raw[0];  // (a list may take several tile rounds: a failed pair of any of them fails the traversal)
    }
  }
  wave_lds_fence();  // praw is written
  return __ballot(bad) == 0;
}

// hnsw.rs:336-372.  0, or kErrOverflow.
template <int OP, int ORDER, bool STAGED>
__device__ __forceinline__ int greedy_closest(const Trav &t, uint32_t *entry, uint32_t layer) {
  uint32_t current = *entry;
  if (t.lane == 0) t.pend[0] = current;
  if (!eval_pending<OP, ORDER, STAGED>(t, 1)) return kErrOverflow;
  float current_dist = rank_of(t.metric, t.praw[0]);
  for (;;) {
    bool moved = false;
    uint32_t count;
    const uint32_t *list = list_of(t.g, current, layer, &count);  // the list of the node current at the top of the pass
    for (uint32_t base = 0; base < count; base += kWave) {
      const uint32_t m = count - base < (uint32_t)kWave ? count - base : (uint32_t)kWave;
      wave_lds_fence();  // the readers of pend / praw are done
      if (t.lane < m) t.pend[t.lane] = list[base + t.lane];
      if (!eval_pending<OP, ORDER, STAGED>(t, m)) return kErrOverflow;
      for (uint32_t j = 0; j < m; ++j) {  // in list order, wave-uniform
        const float dist = rank_of(t.metric, t.praw[j]);
        if (dist < current_dist) {  // IEEE: -0 is not < +0
          current = t.pend[j];
          current_dist = dist;
          moved = true;
        }
      }
    }
    if (!moved) break;
  }
  *entry = current;
  return 0;
}

// hnsw.rs:375-434: leaves the results in t.res[0 .. *rn).  0, kErrOverflow or kHnswRetry.
template <int OP, int ORDER, bool STAGED>
__device__ __forceinline__ int search_layer(const Trav &t, uint32_t entry, uint32_t layer, uint32_t ef, uint32_t *rn_out) {
  const uint32_t lane = t.lane;
  if (ef > t.cap) return kHnswRetry;
  for (uint32_t i = lane; i < 2 * t.cap; i += kWave) t.visited[i] = kNoRow;  // the visited set is fresh per call
  __threadfence();
  wave_lds_fence();
  if (lane == 0) t.pend[0] = entry;
  if (!eval_pending<OP, ORDER, STAGED>(t, 1)) return kErrOverflow;
  uint32_t cn = 0, rn = 0, vcount = 1;  // cn, rn: lane 0's
  if (lane == 0) {
    const uint64_t k = make_key(rank_of(t.metric, t.praw[0]), entry);
    min_push(t.cand, cn, k);
    max_push(t.res, rn, k);
    t.visited[(entry * 2654435761u) >> t.hshift] = entry;
  }
  __threadfence();
  int status = 0;
  for (;;) {
    uint32_t done = 0, cur = 0;
    float worst = 0.0f;
    if (lane == 0) {
      if (cn == 0) {
        done = 1;
      } else {
        const uint64_t k = min_pop(t.cand, cn);
        cur = (uint32_t)k;
        worst = key_dist(t.res[0]);  // read once per popped candidate, not refreshed in the neighbour loop
        if (rn >= ef && key_dist(k) > worst) done = 1;
      }
    }
    done = __shfl(done, 0, kWave);
    if (done) break;
    cur = __shfl(cur, 0, kWave);
    worst = __shfl(worst, 0, kWave);
    uint32_t count;
    const uint32_t *list = list_of(t.g, cur, layer, &count);
    for (uint32_t base = 0; base < count && !status; base += kWave) {
      const uint32_t m = count - base < (uint32_t)kWave ? count - base : (uint32_t)kWave;
      if (vcount + m > t.cap) {
        status = kHnswRetry;
        break;
      }
      // a neighbour is marked visited whether or not it is accepted; the ones that were not yet are the pending list
      bool fresh = false;
      uint32_t nb = kNoRow;
      if (lane < m) {
        nb = list[base + lane];
        uint32_t h = (nb * 2654435761u) >> t.hshift;
        for (;;) {
          const uint32_t old = atomicCAS(&t.visited[h], kNoRow, nb);
          if (old == kNoRow) {
            fresh = true;
            break;
          }
          if (old == nb) break;
          h = (h + 1) & (2 * t.cap - 1);
        }
      }
      const uint64_t mask = __ballot(fresh);
      const uint32_t mf = (uint32_t)__popcll(mask);
      if (mf == 0) continue;
      vcount += mf;
      wave_lds_fence();  // lane 0 is done with the previous pending list
      if (fresh) t.pend[__popcll(mask & ((1ull << lane) - 1))] = nb;
      if (!eval_pending<OP, ORDER, STAGED>(t, mf)) {
        status = kErrOverflow;
        break;
      }
      uint32_t full = 0;
      if (lane == 0) {
        for (uint32_t j = 0; j < mf; ++j) {  // in list order
          const float dist = rank_of(t.metric, t.praw[j]);
          if (rn < ef || dist < worst) {
            if (cn >= t.cap) {
              full = 1;
              break;
            }
            const uint64_t k = make_key(dist, t.pend[j]);
            min_push(t.cand, cn, k);
            // results.push, and results.pop when that made ef + 1: the largest of them goes, the new one or the top
            if (rn < ef) max_push(t.res, rn, k);
            else if (k < t.res[0]) max_replace_top(t.res, rn, k);
          }
        }
      }
      if (__shfl(full, 0, kWave)) status = kHnswRetry;
    }
    if (status) break;
  }
  __threadfence();
  *rn_out = __shfl(rn, 0, kWave);
  return status;
}

template <int OP, int ORDER, bool STAGED>
__global__ __launch_bounds__(kWave) void hnsw_traverse_kernel(const HnswTravArgs a) {
  extern __shared__ __align__(16) float lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t slot = blockIdx.x;
  const uint32_t qi = a.qmap ? a.qmap[slot] : slot;
  const float *qsrc = a.Q + (size_t)qi * a.q_stride;
  uint32_t *out = a.out + (size_t)qi * a.out_stride;

  Trav t;
  t.g = a.g;
  t.metric = a.metric;
  t.lane = lane;
  t.pend = reinterpret_cast<uint32_t *>(lds);
  t.praw = lds + kWave;
  float *qs = lds + 2 * kWave;
  const uint32_t qfl = STAGED ? round_up(a.g.d, 4) : 0;
  t.tile = qs + qfl;
  t.tt = a.tt;
  t.ld = a.ld;
  if (STAGED) {
    for (uint32_t i = lane; i < a.g.d; i += kWave) qs[i] = qsrc[i];
    t.q = qs;
  } else {
    t.q = qsrc;
  }
  t.cap = a.cap;
  t.hshift = a.hshift;
  uint64_t *sc = a.scratch + (size_t)slot * 3 * a.cap;
  t.cand = sc;
  t.res = sc + a.cap;
  t.visited = reinterpret_cast<uint32_t *>(sc + 2 * (size_t)a.cap);
  wave_lds_fence();

  uint32_t entry = a.entry;
  int status = 0;
  const uint32_t first_search = a.mode == 0 ? 0u : (a.node_level < a.top ? a.node_level : a.top);
  for (uint32_t layer = a.top; layer > first_search && !status; --layer)
    status = greedy_closest<OP, ORDER, STAGED>(t, &entry, layer);

  if (a.mode == 0) {
    uint32_t rn = 0;
    if (!status) status = search_layer<OP, ORDER, STAGED>(t, entry, 0, a.ef, &rn);
    // every result as (row, raw): compute()'s value from the same chain, once more
    for (uint32_t j0 = 0; j0 < rn && !status; j0 += kWave) {
      const uint32_t m = rn - j0 < (uint32_t)kWave ? rn - j0 : (uint32_t)kWave;
      wave_lds_fence();
      if (lane < m) t.pend[lane] = (uint32_t)__hip_atomic_load(&t.res[j0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!eval_pending<OP, ORDER, STAGED>(t, m)) {
        status = kErrOverflow;
        break;
      }
      if (lane < m) {
        out[2 + 2 * (j0 + lane)] = t.pend[lane];
        out[3 + 2 * (j0 + lane)] = __float_as_uint(t.praw[lane]);
      }
    }
    if (lane == 0) {
      out[0] = (uint32_t)status;
      out[1] = status ? 0u : rn;
    }
    return;
  }

  // an insert: every layer's result list, (row, rank distance bits); the next layer enters at the list's minimum
  const uint32_t block = 1 + 2 * a.ef;
  for (uint32_t up = 0; up <= first_search && !status; ++up) {
    const uint32_t layer = first_search - up;
    uint32_t rn = 0;
    status = search_layer<OP, ORDER, STAGED>(t, entry, layer, a.ef, &rn);
    if (status) break;
    uint32_t *o = out + 2 + (size_t)layer * block;
    uint32_t best = entry;
    if (lane == 0) {
      uint64_t kmin = ~0ull;
      for (uint32_t i = 0; i < rn; ++i) {
        const uint64_t k = t.res[i];
        kmin = k < kmin ? k : kmin;
        o[1 + 2 * i] = (uint32_t)k;
        o[2 + 2 * i] = __float_as_uint(key_dist(k));
      }
      o[0] = rn;
      best = (uint32_t)kmin;
    }
    entry = __shfl(best, 0, kWave);
  }
  if (lane == 0) {
    out[0] = (uint32_t)status;
    out[1] = first_search + 1;
  }
}

// dst[p.dst] = p.val in the array p.target names: the mirror is patched, not uploaded again
__global__ void hnsw_patch_kernel(const HnswPatch *p, uint32_t n, uint32_t *adj0, uint32_t *upper, uint32_t *level, uint32_t *upoff) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HnswPatch r = p[i];
  uint32_t *dst = r.target == 0 ? adj0 : r.target == 1 ? upper : r.target == 2 ? level : upoff;
  dst[r.dst] = r.val;
}

// ---- K11c: compaction (vt_device.h: HnswCompactArgs).  Four small kernels in stream order behind two memsets: the
// remap table, the rows with level and offset, the layer-0 lists, the upper-layer lists.  A thread owns one 16-byte
// unit of a row or one word of a list; consecutive threads take consecutive units / words, so the stores are dense
// and the loads are dense within a row (1-12 KB) or a list.

// where new row i's upper-layer lists end
__device__ __forceinline__ uint64_t compact_upper_end(const HnswCompactArgs &a, uint32_t i) {
  return i + 1 < a.rows ? (uint64_t)a.new_upoff[i + 1] : a.new_upper;
}

// true: old row s carries `words` words of upper-layer lists, as the plan says, and they lie inside the old array
__device__ __forceinline__ bool compact_shape_ok(const HnswCompactArgs &a, uint32_t s, uint64_t words) {
  if ((uint64_t)a.level[s] * (a.m + 1) != words) return false;
  return words == 0 || (uint64_t)a.upoff[s] + words <= a.old_upper;
}

__global__ void hnsw_remap_kernel(const HnswCompactArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.rows) return;
  const uint32_t s = a.src[i];
  if (s >= a.old_rows) {
    a.status[kHnswCompactShape] = 1;
    return;
  }
  a.remap[s] = i;
}

__global__ void hnsw_compact_rows_kernel(const HnswCompactArgs a, uint32_t rs4) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= (size_t)a.rows * rs4) return;
  const uint32_t i = (uint32_t)(u / rs4), c = (uint32_t)(u % rs4);
  const uint32_t s = a.src[i];
  const bool there = s < a.old_rows;
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (there) v = reinterpret_cast<const f32x4 *>(a.X)[(size_t)s * rs4 + c];
  reinterpret_cast<f32x4 *>(a.outX)[u] = v;
  if (c == 0) {
    const uint64_t words = compact_upper_end(a, i) - a.new_upoff[i];
    if (there && !compact_shape_ok(a, s, words)) a.status[kHnswCompactShape] = 1;
    a.out_level[i] = (uint32_t)(words / (a.m + 1));  // (the plan's level: the mirror's, or the shape guard fired)
    a.out_upoff[i] = a.new_upoff[i];
  }
}

// word `pos` of a list's new image: the count (clamped to lim), the entries renumbered, zeros behind them
__device__ __forceinline__ uint32_t compact_list_word(const HnswCompactArgs &a, const uint32_t *list, uint32_t lim, uint32_t pos) {
  uint32_t cnt = list[0];
  if (cnt > lim) {
    a.status[kHnswCompactCount] = 1;
    cnt = lim;
  }
  if (pos == 0) return cnt;
  if (pos > cnt) return 0;
  const uint32_t e = list[pos];
  if (e >= a.old_rows) {  // before the table is read
    a.status[kHnswCompactBeyond] = 1;
    return kHnswNoRow;
  }
  const uint32_t r = a.remap[e];
  if (r == kHnswNoRow) a.status[kHnswCompactDead] = 1;
  return r;
}

__global__ void hnsw_compact_adj0_kernel(const HnswCompactArgs a) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ls = a.m0 + 1;
  if (u >= (size_t)a.rows * ls) return;
  const uint32_t i = (uint32_t)(u / ls), pos = (uint32_t)(u % ls);
  const uint32_t s = a.src[i];
  a.out_adj0[u] = s < a.old_rows ? compact_list_word(a, a.adj0 + (size_t)s * ls, a.m0, pos) : 0u;
}

__global__ void hnsw_compact_upper_kernel(const HnswCompactArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.new_upper) return;
  // the row whose lists hold word w: the last one that starts at or before it (rows of level 0 hold no word)
  uint32_t lo = 0, hi = a.rows;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)a.new_upoff[mid] <= w) lo = mid;
    else hi = mid;
  }
  const uint32_t i = lo, s = a.src[i];
  const uint64_t first = a.new_upoff[i], words = compact_upper_end(a, i) - first, off = w - first;
  uint32_t out = 0;
  if (s < a.old_rows && first <= w && off < words && compact_shape_ok(a, s, words)) {
    const uint32_t ls = a.m + 1;
    const uint32_t layer = (uint32_t)(off / ls), pos = (uint32_t)(off % ls);
    out = compact_list_word(a, a.upper + (size_t)a.upoff[s] + (size_t)layer * ls, a.m, pos);
  }
  a.out_upper[w] = out;
}

template <int OP, int ORDER>
hipError_t launch_t(const HnswTravArgs &a, uint32_t nslots, hipStream_t s) {
  const bool staged = a.tt != 0;
  const size_t lds = hnsw_lds_bytes(a.g.d, a.tt, a.ld);
  if (staged) hipLaunchKernelGGL((hnsw_traverse_kernel<OP, ORDER, true>), dim3(nslots), dim3(kWave), lds, s, a);
  else hipLaunchKernelGGL((hnsw_traverse_kernel<OP, ORDER, false>), dim3(nslots), dim3(kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dev

void hnsw_tile_plan(uint32_t d, uint32_t stride, uint32_t *tt, uint32_t *ld) {
  *tt = 0;
  *ld = 0;
  if (d > kHnswLdsDim) return;  // rows and query are walked in global memory
  const uint32_t l = (stride / 4) % 2 ? stride : stride + 4;  // ld / 4 odd: the lanes' 16-byte reads of a column spread over the banks
  const size_t room = 64 * 1024 - 2 * dev::kWave * sizeof(float) - (size_t)dev::round_up(d, 4) * sizeof(float);
  uint32_t t = 64;
  while (t > 1 && (size_t)t * l * sizeof(float) > room) t >>= 1;
  *tt = t;
  *ld = l;
}

size_t hnsw_lds_bytes(uint32_t d, uint32_t tt, uint32_t ld) {
  size_t fl = 2 * dev::kWave;
  if (tt) fl += dev::round_up(d, 4) + (size_t)tt * ld;
  return fl * sizeof(float);
}

hipError_t launch_hnsw_traverse(const HnswTravArgs &a, uint32_t nslots, hipStream_t s) {
  using namespace dev;
  if (nslots == 0) return hipSuccess;
  if (a.metric != M_COS && a.metric != M_IP && a.metric != M_L2) return hipErrorInvalidValue;  // (the index's three metrics)
  return dispatch_pair<1u << OP_DOT | 1u << OP_L2 | kPairCosAsDot>(
      a.metric, a.order, [&](auto op, auto order) { return launch_t<op(), order()>(a, nslots, s); });
}

hipError_t launch_hnsw_patch(const HnswPatch *p, uint32_t n, uint32_t *adj0, uint32_t *upper, uint32_t *level, uint32_t *upoff,
                             hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::hnsw_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, n, adj0, upper, level, upoff);
  return hipGetLastError();
}

hipError_t launch_hnsw_compact(const HnswCompactArgs &a, hipStream_t s) {
  if (a.stride == 0 || a.stride % 4 || a.old_rows == kHnswNoRow || a.rows > a.old_rows) return hipErrorInvalidValue;
  constexpr size_t kBlock = 256, kMaxBlocks = 0x7fffffffu;
  const uint32_t rs4 = a.stride / 4;
  const size_t row_blocks = ((size_t)a.rows * rs4 + kBlock - 1) / kBlock;
  const size_t adj_blocks = ((size_t)a.rows * (a.m0 + 1) + kBlock - 1) / kBlock;
  const size_t up_blocks = (size_t)((a.new_upper + kBlock - 1) / kBlock);
  if (row_blocks > kMaxBlocks || adj_blocks > kMaxBlocks || up_blocks > kMaxBlocks) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.status, 0, kHnswCompactGuards * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (a.old_rows && (e = hipMemsetAsync(a.remap, 0xFF, (size_t)a.old_rows * sizeof(uint32_t), s)) != hipSuccess) return e;
  if (a.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::hnsw_remap_kernel, dim3((unsigned)((a.rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(dev::hnsw_compact_rows_kernel, dim3((unsigned)row_blocks), dim3(kBlock), 0, s, a, rs4);
  hipLaunchKernelGGL(dev::hnsw_compact_adj0_kernel, dim3((unsigned)adj_blocks), dim3(kBlock), 0, s, a);
  if (up_blocks) hipLaunchKernelGGL(dev::hnsw_compact_upper_kernel, dim3((unsigned)up_blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace vt

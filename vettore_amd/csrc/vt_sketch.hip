// vt_sketch.hip -- K1q: a lone cosine / dot / L2 search nominated from an int8 sketch of the rows (gfx950), and the tail behind
// its pass -- which K1s and K1f share -- with the threshold, refine and collect kernels behind the nibble sketches' passes
// (K1s, K1f, K1n: vt_sketch_nibble.hip, builders and passes).
//
// The sketch (layout and bounds: vt_device.h, SketchScanArgs) holds a quarter of the f32 rows' bytes.  K1q streams it
// once and gives every row an interval [lo_r, hi_r] that provably holds what K1 would compute for it:
//   * the query arrives as two int8 levels, q ~ t1 Q1 + t2 Q2; v_dot4c_i32_i8 forms Q1.X_r and Q2.X_r exactly in int32;
//   * a_r = s_r (t1 Q1.X_r + t2 Q2.X_r) in f64, e_r = ||q|| rho_r + ||eta|| nu_r + K1's summation error + f64 slack;
//     [a_r - e_r, a_r + e_r] is rounded outwards to f32;
//   * the rank function of the three metrics is monotone non-increasing in the dot, so key(hi_r) <= key_r <= key(lo_r):
//     every block keeps its k' smallest (key(hi_r), id rank) keys (WaveTopK, K1's list layout) with key(lo_r) beside them.
// sketch_tail_kernel then proves that the retained rows with key(hi) <= Kt hold the exact top k and rescores those few
// with K1's exact arithmetic itself; a longer candidate list goes through the gathered K1.
// The L2 family (L2, squared L2) takes the same pass over a column that keeps xx_r >= ||x_r||^2 in the metadata run's free
// dword: ||q - x_r||^2 = ||q||^2 + ||x_r||^2 - 2 q.x_r, so [a_r - e_r, a_r + e_r] (without K1's summation term) gives an
// interval of the real squared distance, K1's f32 value lies within a relative kappa of that, and the two words kept per
// row are kmin_r and kmax_r themselves -- the rank of both metrics is the raw value.
#include "vt_rowscore.cuh"
#include "vt_sketch.cuh"

#include <algorithm>

namespace vt {

namespace {

// One wave per row: quantise, write the row's chunks and its {s, rho, nu} in the tiled layout.  WITH_XX (the L2 family's
// column): sum x^2 in f64 beside the residual, and xx_r -- f32, rounded up, of that sum times 1 + 2^-30 -- in the fourth dword.
template <bool WITH_XX>
__device__ __forceinline__ void sketch_row(const float *__restrict__ X, size_t stride, uint32_t row, bool have_row, uint32_t d,
                                           uint32_t nch, unsigned char *__restrict__ img, unsigned long long *max_norm, int lane) {
  const float *src = X + (size_t)row * stride;
  float m = 0.0f;
  if (have_row)
    for (uint32_t i = lane; i < d; i += kWave) m = fmaxf(m, fabsf(src[i]));
  m = wave_max_f(m);
  float s = m / 127.0f;
  float inv = 127.0f / m;
  const bool quantise = have_row && m > 0.0f && finite_f32(inv) && s > 0.0f;
  if (!quantise) s = 0.0f;
  double res = 0.0;   // sum of (x - s X)^2, f64
  double sq = 0.0;    // sum of x^2, f64 (WITH_XX)
  uint32_t xx = 0;    // sum of X^2, exact
  for (uint32_t c = lane; c < nch; c += kWave) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t i = c * 16 + j * 4 + b;
        const float x = have_row && i < d ? src[i] : 0.0f;
        int q = 0;
        if (quantise) {
          q = (int)rintf(x * inv);
          q = q > 127 ? 127 : (q < -127 ? -127 : q);
        }
        const double r = (double)x - (double)s * (double)q;  // (exact: s q has at most 31 significant bits)
        res += r * r;
        if constexpr (WITH_XX) sq += (double)x * (double)x;
        xx += (uint32_t)(q * q);
        word |= ((uint32_t)q & 0xffu) << (8 * b);
      }
      w[j] = word;
    }
    *reinterpret_cast<u32x4 *>(img + sketch_offset(row, c, nch)) = u32x4{w[0], w[1], w[2], w[3]};
  }
  res = wave_sum_d(res);
  if constexpr (WITH_XX) sq = wave_sum_d(sq);
  xx = wave_sum_u(xx);
  if (lane == 0) {
    // (each f64 sum above carries at most d relative roundings of 2^-53: the 2^-30 margin covers any d this path takes)
    const double rho = sqrt(res) * (1.0 + 0x1p-30);
    const double nu = (double)s * sqrt((double)xx) * (1.0 + 0x1p-30);
    const float rho_f = f32_up(rho), nu_f = f32_up(nu);
    uint32_t xx_w = 0u;
    if constexpr (WITH_XX) xx_w = __float_as_uint(f32_up(sq * (1.0 + 0x1p-30)));
    *reinterpret_cast<u32x4 *>(img + sketch_offset(row, nch, nch)) =
        u32x4{__float_as_uint(s), __float_as_uint(rho_f), __float_as_uint(nu_f), xx_w};
    const double bound = ((double)rho_f + (double)nu_f) * kSlack;
    unsigned long long bits = (unsigned long long)__double_as_longlong(bound);
    atomicMax(max_norm, bits);  // (non-negative f64: the bit patterns order like the values)
  }
}

template <bool WITH_XX>
__global__ __launch_bounds__(256) void sketch_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                           uint32_t rows_img, uint32_t d, uint32_t nch, unsigned char *img,
                                                           unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= rows_img) return;
  sketch_row<WITH_XX>(X, stride, w, w < n_src, d, nch, img, max_norm, threadIdx.x & 63);
}

template <bool WITH_XX>
__global__ __launch_bounds__(256) void sketch_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                          uint32_t count, uint32_t rows_img, uint32_t d, uint32_t nch,
                                                          unsigned char *img, unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= count) return;
  const uint32_t row = list[w];
  if (row >= rows_img) return;
  sketch_row<WITH_XX>(X, stride, row, true, d, nch, img, max_norm, threadIdx.x & 63);
}

// ---- the pass ---------------------------------------------------------------------------------
// A wave owns tiles t = wave, wave + waves, ...; each is nch + 1 one-KiB loads (lane l: row 64 t + l's 16 bytes), kU in
// flight in a register ring that runs on across tiles.  The query's two levels sit in LDS: chunk c's 16 bytes are
// wave-uniform, so a chunk costs one broadcast ds_read_b128 per level and eight v_dot4c_i32_i8.  The tile's last load is
// the rows' metadata: the lane then holds everything its row's interval needs, no other memory access.
// L2: the L2 family's instantiation -- the same loop; the epilogue turns the dot's interval into the two words that hold
// K1's squared distance (or its root), DESIGN 4.10.  The dot family's instantiation is the code it was without it.
template <int CAP, bool L2>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch_scan_kernel(const SketchScanArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t ld8 = a.nch * 16;
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32x4 *qlds = reinterpret_cast<const u32x4 *>(lds_raw);  // [2][nch]
  unsigned char *tkbuf = lds_raw + 2 * ld8 + wib * WaveTopK<CAP>::lds_bytes();
  for (uint32_t i = threadIdx.x; i < 2 * a.nch; i += blockDim.x)
    reinterpret_cast<u32x4 *>(lds_raw)[i] = reinterpret_cast<const u32x4 *>(a.qimg)[i];
  __syncthreads();

  WaveTopK<CAP> tk;
  tk.init(tkbuf, a.k);
  const uint32_t ntiles = (a.n + kSketchTileRows - 1) / kSketchTileRows;
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave = blockIdx.x * kWavesPerBlock + wib;
  const unsigned char *img = static_cast<const unsigned char *>(a.img);
  const uint32_t seg = a.nch + 1;  // loads per tile

  if (wave < ntiles) {
    const uint32_t last_tile = wave + ((ntiles - 1 - wave) / waves) * waves;
    uint32_t pt = wave, pc = 0;  // load cursor
    auto load = [&]() -> u32x4 {
      const uint32_t t = pt < last_tile ? pt : last_tile;  // (past the end: the last tile again, never used)
      const u32x4 v = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4 *>(img + ((size_t)t * seg + pc) * 1024 + (uint32_t)lane * 16));
      if (++pc == seg) {
        pc = 0;
        pt += waves;
      }
      return v;
    };
    u32x4 buf[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) buf[u] = load();

    const double qn = a.qn, eta = a.eta, kerr = a.kerr;
    const double t1 = (double)a.t1, t2 = (double)a.t2;
    // K1's f32 products may be subnormal: an absolute 2^-126 per element covers them, flushed or not
    const double tiny = ((double)a.d + 16.0) * 0x1p-125;
    uint32_t ct = wave, cc = 0;  // compute cursor
    int acc1 = 0, acc2 = 0;
    while (ct < ntiles) {
      bool fin = false;
      int f1 = 0, f2 = 0;
      u32x4 meta = u32x4{0u, 0u, 0u, 0u};
      uint32_t ftile = 0;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const u32x4 x = buf[u];
        buf[u] = load();
        if (ct < ntiles) {
          if (cc < a.nch) {
            const u32x4 q1 = qlds[cc], q2 = qlds[a.nch + cc];
            acc1 = __builtin_amdgcn_sdot4((int)x.x, (int)q1.x, acc1, false);
            acc1 = __builtin_amdgcn_sdot4((int)x.y, (int)q1.y, acc1, false);
            acc1 = __builtin_amdgcn_sdot4((int)x.z, (int)q1.z, acc1, false);
            acc1 = __builtin_amdgcn_sdot4((int)x.w, (int)q1.w, acc1, false);
            acc2 = __builtin_amdgcn_sdot4((int)x.x, (int)q2.x, acc2, false);
            acc2 = __builtin_amdgcn_sdot4((int)x.y, (int)q2.y, acc2, false);
            acc2 = __builtin_amdgcn_sdot4((int)x.z, (int)q2.z, acc2, false);
            acc2 = __builtin_amdgcn_sdot4((int)x.w, (int)q2.w, acc2, false);
            ++cc;
          } else {  // the tile's metadata: the rows are complete (at most one per group: seg > kU)
            fin = true;
            f1 = acc1;
            f2 = acc2;
            meta = x;
            ftile = ct;
            acc1 = acc2 = 0;
            cc = 0;
            ct += waves;
          }
        }
      }
      if (fin) {
        const uint32_t row = ftile * kSketchTileRows + (uint32_t)lane;
        const bool valid = row < a.n;
        const double s = (double)__uint_as_float(meta.x);
        const double rho = (double)__uint_as_float(meta.y), nu = (double)__uint_as_float(meta.z);
        const double av = s * (t1 * (double)f1 + t2 * (double)f2);
        const double e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 0x1p-40 * nu * (qn + eta)) * kSlack + tiny;
        float khi_rank, klo_rank;  // key(lo) >= key(hi): the rank functions fall as the dot rises
        if constexpr (L2) {
          // (kerr = 0: |q.x_r - av| <= e bounds the REAL dot.)  The real ||q - x_r||^2 = qq + xx_r - 2 q.x_r lies in
          // [v_lo, v_hi]; K1's f32 sum of rounded squared differences -- no term negative, nothing cancels -- within
          // kappa = (d + 16) 2^-23 of it, relatively, and `tiny`.  xx_r is the fourth dword: at most 2^-22 above ||x_r||^2.
          const double xxu = (double)__uint_as_float(meta.w), xxl = xxu * (1.0 - 0x1p-22);
          const double kappa = ((double)a.d + 16.0) * 0x1p-23;
          const double delta = 0x1p-40 * (a.qq_hi + xxu + 2.0 * e);
          const double v_lo = fmax(0.0, a.qq_lo + xxl - 2.0 * (av + e) - delta);
          const double v_hi = a.qq_hi + xxu - 2.0 * (av - e) + delta;
          klo_rank = f32_down(v_lo * (1.0 - kappa) - tiny);
          klo_rank = klo_rank > 0.0f ? klo_rank : 0.0f;  // (+0.0: K1's sum of squares is never below it)
          khi_rank = f32_up(v_hi * (1.0 + kappa) + tiny);
          if (a.metric == M_L2) {  // K1's own root: correctly rounded, hence monotone
            klo_rank = __builtin_sqrtf(klo_rank);
            khi_rank = __builtin_sqrtf(khi_rank);
          }
        } else {
          const float hi = f32_up(av + e), lo = f32_down(av - e);
          if (a.metric == M_COS) {
            klo_rank = 1.0f - hi;
            khi_rank = 1.0f - lo;
          } else {
            klo_rank = -hi;
            khi_rank = -lo;
          }
        }
        const uint32_t rank = valid ? (a.id_rank ? a.id_rank[row] : row) : 0u;
        const uint64_t key = ((uint64_t)orderable(klo_rank) << 32) | rank;
        tk.offer(valid, key, row, khi_rank, lane);
      }
    }
  }
  __shared__ uint32_t s_counts[kWavesPerBlock];
  tk.merge_block(wib, kWavesPerBlock, s_counts, lane);
  if (wib == 0) tk.store(a.part_keys + (size_t)blockIdx.x * a.k, a.part_pay + (size_t)blockIdx.x * a.k, lane);
}

// ---- K1q's tail: certification and, for a short candidate list, the exact rescoring and the final select -------------
// One block (K1s and K1f spread the same certification over the card: sketch_thresh_kernel and sketch_collect_kernel
// below).  Kt is the k-th smallest retained key(lo), exactly DESIGN 4.10's threshold.  One sweep of independent loads stages the key(lo) words in LDS when lists * k' of them fit (104 KB at the headline; otherwise later sweeps read
// global memory again) and leaves every thread the smallest of its own; an empty slot counts as 0xffffffff.  The k-th
// smallest of those 1 024 minima is located to its top 16 bits by two 8-bit radix passes over one word per thread; U is
// that bin's upper end.  k distinct entries are <= U, so the entries <= U hold the k smallest of all: they are filed and
// Kt is their k-th smallest by counting (at most 1 024; when more tie around the k-th, Kt is found by four radix passes
// over every word instead).  With k or fewer live entries Kt is the maximum.  The collect is one more sweep of independent loads over the 64-bit keys, its counters (all the
// candidates; each list's own, exact) raised once per wave, not once per candidate; a list is refused when
// every one of its k' slots is a candidate (it is full and its largest key(hi) is <= Kt: it may have dropped a row that
// matters).
// Up to kTailFuseMax candidates whose chunk sums fit the same LDS are then rescored here with K1's arithmetic: a wave
// per row, a lane pair per 8-float chunk (elem4 / chunk_sum of vt_scan.cuh in the index's reduce order), the sums to an
// LDS row, and one thread per candidate walks its row's sums in order -- the reference's sequential chain -- then the
// scalar tail, K1's finiteness check, f64 recovery and status word.  The k best by (rank key, id rank) go sorted into
// the pinned result block like select_topk_kernel's short-list path.  Longer candidate lists are left in rows[] for the
// gathered K1 (info[0] = 2).
constexpr int kTailThreads = 1024;
constexpr uint32_t kTailFuseMax = 256;
constexpr uint32_t kTailSurvivors = 1024;  // entries <= U the exact choice of Kt takes (one per thread)

// hist[bin] += 1 for the lanes with `on`; called by whole waves.  The top digits of the retained keys are nearly all
// equal, and 64 LDS atomics on one address run one after the other: the first two distinct bins of a wave are counted
// by ballot and added once each, whatever is left goes lane by lane.
__device__ __forceinline__ void hist_add(uint32_t *hist, bool on, uint32_t bin, int lane) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint64_t act = __ballot(on);
    if (!act) return;
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)bin, leader, kWave);
    const uint64_t same = __ballot(on && bin == lb);
    if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
    on = on && bin != lb;
  }
  if (on) atomicAdd(&hist[bin], 1u);
}

// A place in a list that *counter counts, for each lane with `on`: the wave's lanes are counted by ballot and the counter
// takes one atomic per wave, not one per lane (thousands of candidates behind the 5-bit pass would queue on it).  Called
// by the lanes of a wave that are in the loop together; a lane without `on` gets nothing it may use.
__device__ __forceinline__ uint32_t wave_claim(uint32_t *counter, bool on, int lane) {
  const uint64_t act = __ballot(on);
  if (!act) return 0u;
  const int leader = __ffsll((long long)act) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(act));
  base = (uint32_t)__shfl((int)base, leader, kWave);
  return base + (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
}

// Wave 0 of a block, after a radix digit's histogram (256 bins): the bin that holds the *remaining-th smallest of this
// digit joins *prefix_out, and *remaining becomes the rank inside that bin (four bins per lane, one wave scan).
__device__ __forceinline__ void radix_pick_bin(const uint32_t *hist, uint32_t *prefix_out, uint32_t *remaining, uint32_t prefix,
                                               int shift, int lane) {
  const uint32_t krem = *remaining;
  const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
  const uint32_t sum = h0 + h1 + h2 + h3;
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o, kWave);
    if (lane >= o) incl += t;
  }
  uint32_t cum = incl - sum;
  if (cum < krem && krem <= incl) {
    uint32_t b = 0;
    if (cum + h0 < krem) {
      cum += h0;
      b = 1;
      if (cum + h1 < krem) {
        cum += h1;
        b = 2;
        if (cum + h2 < krem) {
          cum += h2;
          b = 3;
        }
      }
    }
    *remaining = krem - cum;
    *prefix_out = prefix | ((4u * (uint32_t)lane + b) << shift);
  }
}

// L2: the L2 family's instantiation rescores with K1's squared differences and, for VT_L2, K1's root.
// (The block's whole work as a function: sketch_tail_kernel runs it on its arguments, sketch_tail_group_kernel -- K1qm's
// tail, a block per query of a group -- on block g's slice of them.)
template <bool L2>
__device__ __forceinline__ void sketch_tail_body(const SketchTailArgs a) {
  extern __shared__ __align__(16) uint32_t dyn[];  // the key(lo) words; once Kt is known: per-list counts, chunk sums
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_remaining, s_total, s_count, s_fail, s_live, s_nsv, s_kt;
  __shared__ uint32_t sv[kTailSurvivors];
  __shared__ uint32_t c_row[kTailFuseMax];
  __shared__ uint64_t c_key[kTailFuseMax];
  const uint32_t m = a.lists * a.kp;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  const bool in_lds = m <= a.lds_words;
  if (tid == 0) {
    s_prefix = 0;
    s_remaining = a.k;
    s_total = 0;
    s_count = 0;
    s_fail = 0;
    s_live = 0;
    s_nsv = 0;
    s_kt = 0xffffffffu;
  }
  __syncthreads();
  constexpr uint32_t kUnroll = 8;
  uint32_t mine = 0xffffffffu;  // the smallest key(lo) word among this thread's entries
  uint32_t live = 0;
  for (uint32_t b = tid; b < m; b += kUnroll * kTailThreads) {
    uint64_t key[kUnroll];
    float raw[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t i = b + u * kTailThreads;
      key[u] = i < m ? a.keys[i] : kEmptyKey;
      raw[u] = i < m ? a.pay[i].raw : 0.0f;  // (an empty slot's payload was never written: loaded, not used)
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t i = b + u * kTailThreads;
      const uint32_t v = key[u] == kEmptyKey ? 0xffffffffu : orderable(raw[u]);
      live += key[u] != kEmptyKey ? 1u : 0u;
      mine = v < mine ? v : mine;
      if (i < m && in_lds) dyn[i] = v;
    }
  }
  live = wave_sum_u(live);
  if (lane == 0 && live) atomicAdd(&s_total, live);
  // U = the upper end of the 16-bit bin that holds the k-th smallest of the 1 024 threads' minima (k <= 256): k distinct
  // entries are <= U, so Kt <= U, and the entries <= U -- a few more than k unless hundreds tie -- hold the k smallest
  // of all.  Two radix passes over one word per thread, in place of four over all lists * k' words.
  uint32_t mask = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    hist_add(hist, (mine & mask) == prefix, (mine >> shift) & 255u, lane);
    __syncthreads();
    if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
    mask |= 255u << shift;
    __syncthreads();
  }
  // the entries <= U into sv[]; Kt = their k-th smallest, every survivor's place found by counting
  uint32_t kt = 0xffffffffu;  // (k or fewer entries in all: every one is a candidate)
  if (s_total > a.k) {
    const uint32_t ub = s_prefix | 0xffffu;
    for (uint32_t b = tid; b < m; b += kUnroll * kTailThreads) {
      uint32_t v[kUnroll];
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u) {
        const uint32_t i = b + u * kTailThreads;
        v[u] = 0xffffffffu;
        if (i < m) v[u] = in_lds ? dyn[i] : (a.keys[i] == kEmptyKey ? 0xffffffffu : orderable(a.pay[i].raw));
      }
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u) {
        if (b + u * kTailThreads < m && v[u] <= ub) {
          const uint32_t pos = atomicAdd(&s_nsv, 1u);
          if (pos < kTailSurvivors) sv[pos] = v[u];
        }
      }
    }
    __syncthreads();
    const uint32_t nsv = s_nsv;
    if (nsv > kTailSurvivors) {
      // Over a thousand entries <= U: they tie around the k-th (thousands of copies of one row behind the 5-bit pass, whose
      // candidate list has room for them).  Kt is then the k-th smallest word itself, by four radix passes over every word.
      if (tid == 0) {
        s_prefix = 0;
        s_remaining = a.k;
      }
      uint32_t rmask = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (uint32_t i = tid; i < m; i += kTailThreads) {
          const uint32_t v = in_lds ? dyn[i] : (a.keys[i] == kEmptyKey ? 0xffffffffu : orderable(a.pay[i].raw));
          hist_add(hist, (v & rmask) == prefix, (v >> shift) & 255u, lane);
        }
        __syncthreads();
        if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
        rmask |= 255u << shift;
        __syncthreads();
      }
      if (tid == 0) s_kt = s_prefix;
    } else if (tid < nsv) {
      const uint32_t v = sv[tid];
      uint32_t lt = 0, le = 0;
      for (uint32_t x = 0; x < nsv; ++x) {
        const uint32_t o = sv[x];
        lt += o < v ? 1u : 0u;
        le += o <= v ? 1u : 0u;
      }
      if (lt < a.k && a.k <= le) s_kt = v;  // (every thread that gets here writes the same word)
    }
    __syncthreads();
    kt = s_kt;
  }

  // collect; dyn[0..lists): candidates per list
  const uint32_t lists4 = (a.lists + 3u) & ~3u;
  for (uint32_t l = tid; l < a.lists; l += kTailThreads) dyn[l] = 0;
  __syncthreads();
  for (uint32_t b = tid; b < m; b += kUnroll * kTailThreads) {
    uint64_t key[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t i = b + u * kTailThreads;
      key[u] = i < m ? a.keys[i] : kEmptyKey;
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      const uint32_t i = b + u * kTailThreads;
      const bool cand = key[u] != kEmptyKey && (uint32_t)(key[u] >> 32) <= kt;
      const uint32_t pos = wave_claim(&s_count, cand, lane);
      if (cand) {
        const uint32_t row = a.pay[i].row;
        if (pos < a.cap) a.rows[pos] = row;
        if (pos < kTailFuseMax) c_row[pos] = row;
      }
      hist_add(dyn, cand, i / a.kp, lane);
    }
  }
  __syncthreads();
  for (uint32_t l = tid; l < a.lists; l += kTailThreads)
    if (dyn[l] == a.kp) s_fail = 1;
  __syncthreads();
  const uint32_t cnt = s_count;
  const bool ok = !s_fail && cnt <= a.cap;
  const bool fused = ok && cnt <= kTailFuseMax && lists4 + cnt * a.ss <= a.lds_words;
  if (!fused) {
    if (tid == 0) {
      *a.count = ok ? cnt : 0u;
      a.info[0] = ok ? 2u : 0u;
      a.info[1] = cnt;
      a.info[2] = kt;
      a.info[3] = 0u;
    }
    return;
  }

  // K1 on the candidates: wave w takes candidates w, w + 16, ...; lane l the floats [256 s + 4 l, + 4) of segment s
  float *S = reinterpret_cast<float *>(dyn + lists4);  // [cnt][ss]
  constexpr int OP = L2 ? OP_L2 : OP_DOT;
  const int odd = lane & 1;
  const uint32_t cfull = a.d / 8, tail = a.d % 8, tail_base = a.ss - 12;
  for (uint32_t c = (uint32_t)w; c < cnt; c += kTailThreads / kWave) {
    const float *x = a.X + (size_t)c_row[c] * a.stride;
    float *Srow = S + (size_t)c * a.ss;
    for (uint32_t s0 = 0; s0 < a.ld; s0 += 4 * 256) {
      f32x4 xv[4], qv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t col = s0 + u * 256 + (uint32_t)lane * 4;
        const bool in = col < a.ld;
        xv[u] = in ? *reinterpret_cast<const f32x4 *>(x + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        qv[u] = in ? *reinterpret_cast<const f32x4 *>(a.q + col) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t col = s0 + u * 256 + (uint32_t)lane * 4;
        const f32x4 pr = elem4<OP>(OP, qv[u], xv[u]);
        const float sum = chunk_sum<OP, -1>(OP, a.order, pr.x, pr.y, pr.z, pr.w, odd);
        const uint32_t ch = col >> 3;
        if (col < a.ld) {
          if (ch < cfull) {
            if (!odd) Srow[ch] = sum;
          } else if (ch == cfull) {  // the tail chunk: the reference adds these products one by one
            *reinterpret_cast<f32x4 *>(Srow + tail_base + odd * 4) = pr;
          }
        }
      }
    }
  }
  __syncthreads();
  uint64_t key = kEmptyKey;
  uint32_t row = 0;
  float raw = 0.0f;
  if (tid < cnt) {
    row = c_row[tid];
    const float *Sr = S + (size_t)tid * a.ss;
    float acc = 0.0f;
    uint32_t c = 0;
    for (; c + 4 <= cfull; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(Sr + c);
      acc = acc + v.x;
      acc = acc + v.y;
      acc = acc + v.z;
      acc = acc + v.w;
    }
    for (; c < cfull; ++c) acc = acc + Sr[c];
    for (uint32_t j = 0; j < tail; ++j) acc = acc + Sr[tail_base + j];
    // distances.rs:42-68 compute(): value, finiteness, f64 recovery -- as scan_topk_kernel has them
    if constexpr (L2) raw = a.metric == M_L2 && finite_f32(acc) ? __builtin_sqrtf(acc) : acc;
    else raw = a.metric == M_NIP ? -acc : acc;
    bool valid = true;
    if (!finite_f32(raw)) {
      const float rec = recover_overflow(a.metric, a.q, a.X + (size_t)row * a.stride, a.d);
      if (rec == rec) {
        raw = rec;
      } else {
        atomicMax(a.status, kErrOverflow);
        valid = false;
      }
    }
    float rank = raw;  // (the L2 family ranks by the raw value)
    if constexpr (!L2) {
      if (a.metric == M_COS) rank = 1.0f - raw;
      else if (a.metric == M_IP) rank = -raw;
    }
    if (valid) key = ((uint64_t)orderable(rank) << 32) | (a.id_rank ? a.id_rank[row] : row);
  }
  if (tid < kTailFuseMax) c_key[tid] = key;
  const uint64_t votes = __ballot(key != kEmptyKey);
  if (lane == 0 && votes) atomicAdd(&s_live, (uint32_t)__popcll(votes));
  __syncthreads();
  if (key != kEmptyKey) {
    uint32_t pos = 0;
    for (uint32_t x = 0; x < cnt; ++x) {
      const uint64_t kx = c_key[x];
      pos += (kx < key || (kx == key && x < tid)) ? 1u : 0u;
    }
    if (pos < a.k) {
      Entry e;
      e.key = key;
      e.row = row;
      e.raw = raw;
      a.out->e[pos] = e;
    }
  }
  if (tid == 0) {
    a.out->count = s_live < a.k ? s_live : a.k;
    a.out->status = atomicExch(a.status, 0);  // (every atomicMax above is behind the barrier)
    *a.count = cnt;
    a.info[0] = 1u;
    a.info[1] = cnt;
    a.info[2] = kt;
    a.info[3] = 0u;
  }
}

template <bool L2>
__global__ __launch_bounds__(kTailThreads) void sketch_tail_kernel(const SketchTailArgs a) {
  sketch_tail_body<L2>(a);
}

// K1qm's tail: block g is launch_sketch_tail's one block on query g's lists, rows, count, info, query, result and status.
template <bool L2>
__global__ __launch_bounds__(kTailThreads) void sketch_tail_group_kernel(const SketchTailArgs a0, size_t q_stride) {
  const uint32_t g = blockIdx.x;
  SketchTailArgs a = a0;
  a.keys += (size_t)g * a0.lists * a0.kp;
  a.pay += (size_t)g * a0.lists * a0.kp;
  a.rows += (size_t)g * a0.cap;
  a.count += g;
  a.info += 4 * g;
  a.q += (size_t)g * q_stride;
  a.status += g;
  a.out += g;
  sketch_tail_body<L2>(a);
}

// ---- the tail of K1s and K1f, spread over the card: two kernels, Kt across the boundary between them ------------------
// Behind these passes nothing is rescored by the certifying block (hundreds to tens of thousands of candidates: the
// gathered K1 and its select are queued behind), and the lists' words arrive a second time as two plain arrays
// (SketchSpreadArgs::lo_words / hi_words).  One block sweeping lists * k' words three times left the other CUs idle for
// its whole duration; here every block owns a slice, and nothing waits inside a kernel.
//   sketch_thresh_kernel   block b: the k smallest key(lo) words of slots [b * kThreshSlots, + kThreshSlots), with
//                          multiplicity, to parts[b][0..k) in any order, and the slice's live words to live[b].  An empty
//                          slot (and a slot past the end) counts as 0xffffffff, so a slice with fewer than k live words
//                          pads with that word.  Four 8-bit radix passes over the thread's own words find the slice's k-th
//                          smallest word v and how many copies of it belong to the k: the words < v are filed by wave_claim,
//                          v is written as often as is left.  The k smallest of all the slots are among the slices' k
//                          smallest, so Kt = the k-th smallest word of parts[], exactly.  Block 0 zeroes the three words
//                          the collect shares (claim, fail, ticket): every call starts from zero whatever the last one did.
//   sketch_collect_kernel  every block finds Kt for itself from parts[] (at most a few thousand words, staged in LDS; four
//                          radix passes; 0xffffffff when k or fewer words are live) -- cheaper than a third kernel --, then
//                          sweeps the key(hi) words of its own whole lists: a slot is a candidate iff h != 0xffffffff and
//                          h <= Kt.  The candidates' rows are staged in LDS at places wave_claim hands out on an LDS
//                          counter; the block then takes ONE returning atomic on the claim word for all of them and
//                          copies them to rows[base ..) (pos < cap).  One word takes about 88 atomics a us: one per wave
//                          of the sweep (1 024) would queue for over 10 us, one per block for under 3.  A list whose k'
//                          slots are all candidates raises the fail word (per-list counts exact, through hist_add).
// The one exchange inside a launch (kernel guide, Guideline 16): count and info[] need every block's claim.  Each block,
// its atomics and stores drained by every wave and behind a block barrier, has one lane issue an agent-scope release and
// draw a ticket with a returning atomic; the block that draws the last one reads the claim total and the fail word through
// returning agent-scope atomics alone (never a plain load, never the scalar path) and writes *count = ok ? cnt : 0 and
// info = {ok ? 2 : 0, cnt, Kt, 1}, ok = !fail && cnt <= cap.  Nothing polls: a block that is not last just ends.  The
// order of rows[] across blocks is whatever the claims make it; the gathered K1 keeps per-block lists and the select
// orders by (rank key, id rank), so it reaches no result.
constexpr int kSpreadThreads = 256;
constexpr uint32_t kThreshSlots = 1024;                                  // a threshold block's slice
constexpr uint32_t kThreshPer = kThreshSlots / (uint32_t)kSpreadThreads;  // words per thread
constexpr uint32_t kCollectLists = 16;                                   // whole lists per collect block (more when over kCollectMaxBlocks)
constexpr uint32_t kCollectMaxBlocks = 256;

__device__ __forceinline__ uint32_t agent_add(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kSpreadThreads) void sketch_thresh_kernel(const SketchSpreadArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_remaining, s_live, s_out, s_eq;
  const uint32_t m = a.lists * a.kp;
  const uint32_t tid = threadIdx.x, base = blockIdx.x * kThreshSlots;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  if (blockIdx.x == 0 && tid < 3) __hip_atomic_store(a.sync + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    s_prefix = 0;
    s_remaining = a.k;
    s_live = 0;
    s_out = 0;
    s_eq = 0;
  }
  uint32_t v[kThreshPer];
  uint32_t live = 0;
#pragma unroll
  for (uint32_t u = 0; u < kThreshPer; ++u) {
    const uint32_t i = base + u * kSpreadThreads + tid;
    v[u] = i < m ? a.lo_words[i] : 0xffffffffu;
  }
#pragma unroll
  for (uint32_t u = 0; u < kThreshPer; ++u) live += v[u] != 0xffffffffu ? 1u : 0u;
  live = wave_sum_u(live);
  __syncthreads();
  if (lane == 0 && live) atomicAdd(&s_live, live);
  uint32_t mask = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
#pragma unroll
    for (uint32_t u = 0; u < kThreshPer; ++u) hist_add(hist, (v[u] & mask) == prefix, (v[u] >> shift) & 255u, lane);
    __syncthreads();
    if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
    mask |= 255u << shift;
    __syncthreads();
  }
  // vk: the slice's k-th smallest word; `need` of its copies belong to the k (k - need words are smaller)
  const uint32_t vk = s_prefix, need = s_remaining;
  uint32_t *out = a.parts + (size_t)blockIdx.x * a.k;
#pragma unroll
  for (uint32_t u = 0; u < kThreshPer; ++u) {
    const bool below = v[u] < vk;
    const uint32_t pos = wave_claim(&s_out, below, lane);
    if (below && pos < a.k) out[pos] = v[u];
    if (a.slots && below && pos < a.k) a.slots[(size_t)blockIdx.x * a.k + pos] = base + u * kSpreadThreads + tid;
  }
  if (tid < need && need <= a.k) out[a.k - need + tid] = vk;
  if (a.slots && need <= a.k) {
    // the copies of vk: `need` distinct slots that hold it (a padded slice files empty slots, past the end included:
    // their word says so)
    uint32_t *sl = a.slots + (size_t)blockIdx.x * a.k + (a.k - need);
#pragma unroll
    for (uint32_t u = 0; u < kThreshPer; ++u) {
      const bool eq = v[u] == vk;
      const uint32_t pos = wave_claim(&s_eq, eq, lane);
      if (eq && pos < need) sl[pos] = base + u * kSpreadThreads + tid;
    }
  }
  if (tid == 0) a.live[blockIdx.x] = s_live;
}

// ---- K1n's threshold from exact rescoring (vt_device.h, SketchRefineArgs) ---------------------------------
// One block between the two kernels.  Kt and the k smallest (word, slot) pairs of parts[]: four radix passes over the
// words staged in LDS as the collect has them, the words below Kt filed by wave_claim, Kt's copies as often as are left.
// Then sketch_tail_kernel's rescoring on those k rows: a wave per row, a lane pair per 8-float chunk, the sums to an LDS
// row, one thread per row down the reference's sequential chain and the scalar tail.  Nothing waits for another block.
__global__ __launch_bounds__(kTailThreads) void sketch_refine_kernel(const SketchRefineArgs a) {
  extern __shared__ __align__(16) uint32_t dyn[];  // parts[] | slots[] | the k rows' chunk sums
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_remaining, s_live, s_lt, s_eq, s_bad, s_max;
  __shared__ uint32_t sel_slot[kSpreadThreads], sel_row[kSpreadThreads];
  const uint32_t tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  const uint32_t np = a.thresh_blocks * a.k;
  uint32_t *pw = dyn, *ps = dyn + a.np4;
  if (tid == 0) {
    s_prefix = 0;
    s_remaining = a.k;
    s_live = 0;
    s_lt = 0;
    s_eq = 0;
    s_bad = 0;
    s_max = 0;
  }
  if (tid < a.k) sel_slot[tid] = 0xffffffffu;
  for (uint32_t i = tid; i < np; i += kTailThreads) {
    pw[i] = a.parts[i];
    ps[i] = a.slots[i];
  }
  uint32_t live = 0;
  for (uint32_t i = tid; i < a.thresh_blocks; i += kTailThreads) live += a.live[i];
  live = wave_sum_u(live);
  __syncthreads();
  if (lane == 0 && live) atomicAdd(&s_live, live);
  __syncthreads();
  if (s_live <= a.k || a.ss == 0) {  // (k or fewer live words: every one is a candidate, as the collect has it)
    uint32_t kt = 0xffffffffu;
    if (s_live > a.k) {
      // the rows do not fit: Kt itself, by the same four passes
      uint32_t mask = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (uint32_t b = 0; b < np; b += kTailThreads) {
          const uint32_t i = b + tid;
          const uint32_t x = i < np ? pw[i] : 0u;
          hist_add(hist, i < np && (x & mask) == prefix, (x >> shift) & 255u, lane);
        }
        __syncthreads();
        if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
        mask |= 255u << shift;
        __syncthreads();
      }
      kt = s_prefix;
    }
    if (tid == 0) *a.kt_out = kt;
    if (a.picked && tid < a.k) a.picked[tid] = 0xffffffffu;
    return;
  }
  uint32_t mask = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    for (uint32_t b = 0; b < np; b += kTailThreads) {  // (whole waves: hist_add votes)
      const uint32_t i = b + tid;
      const uint32_t x = i < np ? pw[i] : 0u;
      hist_add(hist, i < np && (x & mask) == prefix, (x >> shift) & 255u, lane);
    }
    __syncthreads();
    if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
    mask |= 255u << shift;
    __syncthreads();
  }
  // kt: the k-th smallest word (live: more than k words are); `need` of its copies belong to the k
  const uint32_t kt = s_prefix, need = s_remaining;
  for (uint32_t b = 0; b < np; b += kTailThreads) {  // (whole waves: wave_claim votes)
    const uint32_t i = b + tid;
    const uint32_t x = i < np ? pw[i] : 0xffffffffu;
    const bool below = i < np && x < kt, eq = i < np && x == kt;
    const uint32_t pl = wave_claim(&s_lt, below, lane);
    if (below && pl < a.k) sel_slot[pl] = ps[i];
    const uint32_t pe = wave_claim(&s_eq, eq, lane);
    if (eq && pe < need && need <= a.k) sel_slot[a.k - need + pe] = ps[i];
  }
  __syncthreads();
  if (tid < a.k) {
    const uint32_t slot = sel_slot[tid];
    uint32_t row = 0xffffffffu;
    if (slot < a.slots_total) row = a.pay[slot].row;
    else s_bad = 1;  // (cannot be: a word below 0xffffffff came from a live slot)
    sel_row[tid] = row;
  }
  __syncthreads();
  // K1 on the k rows: wave w takes rows w, w + 16, ...; lane l the floats [256 s + 4 l, + 4) of segment s
  float *S = reinterpret_cast<float *>(dyn + 2 * a.np4);  // [k][ss]
  const int odd = lane & 1;
  const uint32_t cfull = a.d / 8, tail = a.d % 8, tail_base = a.ss - 12;
  for (uint32_t c = (uint32_t)w; c < a.k; c += kTailThreads / kWave) {
    if (sel_row[c] == 0xffffffffu) continue;
    const float *x = a.X + (size_t)sel_row[c] * a.stride;
    float *Srow = S + (size_t)c * a.ss;
    for (uint32_t s0 = 0; s0 < a.ld; s0 += 4 * 256) {
      f32x4 xv[4], qv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t col = s0 + u * 256 + (uint32_t)lane * 4;
        const bool in = col < a.ld;
        xv[u] = in ? *reinterpret_cast<const f32x4 *>(x + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        qv[u] = in ? *reinterpret_cast<const f32x4 *>(a.q + col) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        row_chunk<-1>(Srow, qv[u], xv[u], s0 + u * 256 + (uint32_t)lane * 4, a.ld, cfull, tail_base, a.order, odd);
    }
  }
  __syncthreads();
  if (tid < a.k && sel_row[tid] != 0xffffffffu) {
    // the value and its rank as scan_topk_kernel forms them (vt_rowscore.cuh); a value that is not finite goes through
    // K1's f64 recovery there: here it only means that this call keeps the sketch's own threshold
    uint32_t word;
    if (!row_rank_word(a.metric, row_chain(S + (size_t)tid * a.ss, cfull, tail, tail_base), &word)) s_bad = 1;
    else atomicMax(&s_max, word);
  }
  __syncthreads();
  if (tid == 0) *a.kt_out = s_bad ? kt : (s_max < kt ? s_max : kt);
  if (a.picked && tid < a.k) a.picked[tid] = sel_row[tid];
}

__global__ __launch_bounds__(kSpreadThreads) void sketch_collect_kernel(const SketchSpreadArgs a) {
  extern __shared__ __align__(16) uint32_t dyn[];  // parts[] | the block's candidate rows | its lists' candidate counts
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_remaining, s_live, s_n, s_base;
  const uint32_t tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid / kWave;
  const uint32_t np = a.thresh_blocks * a.k;
  const uint32_t l0 = blockIdx.x * a.collect_lists;
  const uint32_t nl = a.lists - l0 < a.collect_lists ? a.lists - l0 : a.collect_lists;
  const uint32_t slots = nl * a.kp, first = l0 * a.kp;
  uint32_t *pw = dyn, *stage = dyn + ((np + 3u) & ~3u), *lcnt = stage + a.collect_lists * a.kp;
  if (tid == 0) {
    s_prefix = 0;
    s_remaining = a.k;
    s_live = 0;
    s_n = 0;
    s_base = 0;
  }
  for (uint32_t l = tid; l < nl; l += kSpreadThreads) lcnt[l] = 0;
  // Kt from the partial thresholds (plain loads: the kernel boundary has published them)
  uint32_t live = 0;
  if (!a.kt_word) {
    for (uint32_t i = tid; i < np; i += kSpreadThreads) pw[i] = a.parts[i];
    for (uint32_t i = tid; i < a.thresh_blocks; i += kSpreadThreads) live += a.live[i];
  }
  live = wave_sum_u(live);
  __syncthreads();
  if (lane == 0 && live) atomicAdd(&s_live, live);
  __syncthreads();
  uint32_t kt = 0xffffffffu;  // (k or fewer entries in all: every one is a candidate)
  if (a.kt_word) {
    kt = *a.kt_word;  // (K1n: launch_sketch_refine's word, published by the kernel boundary; never above the Kt of parts[])
  } else if (s_live > a.k) {
    uint32_t mask = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      const uint32_t prefix = s_prefix;
      for (uint32_t b = 0; b < np; b += kSpreadThreads) {  // (whole waves: hist_add votes)
        const uint32_t i = b + tid;
        const uint32_t x = i < np ? pw[i] : 0u;
        hist_add(hist, i < np && (x & mask) == prefix, (x >> shift) & 255u, lane);
      }
      __syncthreads();
      if (w == 0) radix_pick_bin(hist, &s_prefix, &s_remaining, prefix, shift, lane);
      mask |= 255u << shift;
      __syncthreads();
    }
    kt = s_prefix;
  }
  // the block's own lists: candidates' rows to LDS, each list's count
  for (uint32_t b = 0; b < slots; b += kSpreadThreads) {  // (whole waves: wave_claim and hist_add vote)
    const uint32_t i = b + tid;
    const uint32_t h = i < slots ? a.hi_words[first + i] : 0xffffffffu;
    const bool cand = h != 0xffffffffu && h <= kt;
    const uint32_t pos = wave_claim(&s_n, cand, lane);
    if (cand) stage[pos] = a.pay[first + i].row;
    hist_add(lcnt, cand, i / a.kp, lane);
  }
  __syncthreads();
  const uint32_t n = s_n;
  if (tid == 0 && n) s_base = agent_add(a.sync + 0, n);  // the block's one claim
  for (uint32_t l = tid; l < nl; l += kSpreadThreads)
    if (lcnt[l] == a.kp) __hip_atomic_fetch_or(a.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint32_t base = s_base;
  for (uint32_t j = tid; j < n; j += kSpreadThreads)
    if (base + j < a.cap) a.rows[base + j] = stage[j];
  // the ticket: every wave's atomics and stores drained, the barrier, one lane's release, then its draw
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ticket = agent_add(a.sync + 2, 1u);
    if (ticket == gridDim.x - 1) {  // every other block has claimed and flagged before it drew
      const uint32_t cnt = agent_add(a.sync + 0, 0u);
      const uint32_t fail = __hip_atomic_fetch_or(a.sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool ok = !fail && cnt <= a.cap;
      *a.count = ok ? cnt : 0u;
      a.info[0] = ok ? 2u : 0u;
      a.info[1] = cnt;
      a.info[2] = kt;
      a.info[3] = 1u;
    }
  }
}

}  // namespace

template <bool WITH_XX>
static hipError_t sketch_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                               unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim || rows_img % kSketchTileRows) return hipErrorInvalidValue;
  if (rows_img == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch_build_kernel<WITH_XX>, dim3((rows_img + 3) / 4), dim3(256), 0, s, X, stride, n_src, rows_img, d,
                     sketch_ld8(d) / 16, static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

template <bool WITH_XX>
static hipError_t sketch_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                              void *img, unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch_rows_kernel<WITH_XX>, dim3((count + 3) / 4), dim3(256), 0, s, X, stride, list, count, rows_img, d,
                     sketch_ld8(d) / 16, static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

hipError_t launch_sketch_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                               unsigned long long *max_norm, hipStream_t s) {
  return sketch_build<false>(X, stride, n_src, rows_img, d, img, max_norm, s);
}
hipError_t launch_sketch_build_xx(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                  unsigned long long *max_norm, hipStream_t s) {
  return sketch_build<true>(X, stride, n_src, rows_img, d, img, max_norm, s);
}
hipError_t launch_sketch_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                              void *img, unsigned long long *max_norm, hipStream_t s) {
  return sketch_rows<false>(X, stride, list, count, rows_img, d, img, max_norm, s);
}
hipError_t launch_sketch_rows_xx(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                                 void *img, unsigned long long *max_norm, hipStream_t s) {
  return sketch_rows<true>(X, stride, list, count, rows_img, d, img, max_norm, s);
}

size_t sketch_scan_lds_bytes(uint32_t d, uint32_t k) {
  if (d == 0 || d > kSketchMaxDim || k == 0 || k > (uint32_t)kMaxFusedK) return 0;
  const size_t buf = k <= (uint32_t)kSmallK ? WaveTopK<kCapSmall>::lds_bytes() : WaveTopK<kCapLarge>::lds_bytes();
  const size_t bytes = 2 * (size_t)sketch_ld8(d) + kWavesPerBlock * buf;
  return bytes <= kMaxLds ? bytes : 0;
}

hipError_t launch_sketch_scan(const SketchScanArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = sketch_scan_lds_bytes(a.d, a.k);
  if (!lds || a.nch != sketch_ld8(a.d) / 16 || blocks == 0 || !a.part_keys || !a.part_pay) return hipErrorInvalidValue;
  const bool l2 = a.metric == M_L2 || a.metric == M_L2SQ;
  if (!l2 && a.metric != M_COS && a.metric != M_IP && a.metric != M_NIP) return hipErrorInvalidValue;
  auto launch = [&](auto kernel) -> hipError_t {
    hipError_t e = allow_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
    return hipGetLastError();
  };
  if (a.k <= (uint32_t)kSmallK) return l2 ? launch(sketch_scan_kernel<kCapSmall, true>) : launch(sketch_scan_kernel<kCapSmall, false>);
  return l2 ? launch(sketch_scan_kernel<kCapLarge, true>) : launch(sketch_scan_kernel<kCapLarge, false>);
}

size_t sketch_tail_lds_bytes(uint32_t lists, uint32_t kp, uint32_t d) {
  // the key(lo) words if they fit, and room for a few dozen rows of chunk sums beside the per-list counts
  const size_t room = 128 * 1024;
  const size_t want = std::max((size_t)lists * kp, ((size_t)lists + 4) + 64 * (size_t)(padded_dim(d) / 8 + 12)) * 4;
  return std::max(std::min(want, room), ((size_t)lists + 4) * 4);
}

hipError_t launch_sketch_tail(SketchTailArgs a, hipStream_t s) {
  if (a.lists == 0 || a.kp == 0 || a.k == 0 || a.k > a.kp || a.k > (uint32_t)kMaxFusedK || !a.rows || !a.count || !a.info || !a.out ||
      !a.status || a.d == 0)
    return hipErrorInvalidValue;
  const size_t lds = sketch_tail_lds_bytes(a.lists, a.kp, a.d);
  if (lds > kMaxLds - 8 * 1024) return hipErrorInvalidValue;
  a.ld = padded_dim(a.d);
  a.ss = a.ld / 8 + 12;  // (K1's panel row: 4 * odd dwords, the eight tail products behind the sums)
  a.lds_words = (uint32_t)(lds / 4);
  const bool l2 = a.metric == M_L2 || a.metric == M_L2SQ;
  if (!l2 && a.metric != M_COS && a.metric != M_IP && a.metric != M_NIP) return hipErrorInvalidValue;
  auto kernel = l2 ? sketch_tail_kernel<true> : sketch_tail_kernel<false>;
  hipError_t e = allow_lds(kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(kTailThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_sketch_tail_group(SketchTailArgs a, uint32_t ng, size_t q_stride, hipStream_t s) {
  if (a.lists == 0 || a.kp == 0 || a.k == 0 || a.k > a.kp || a.k > (uint32_t)kMaxFusedK || !a.rows || !a.count || !a.info || !a.out ||
      !a.status || a.d == 0 || ng == 0 || ng > (uint32_t)kSketchMultiMax || a.cap == 0)
    return hipErrorInvalidValue;
  const size_t lds = sketch_tail_lds_bytes(a.lists, a.kp, a.d);
  if (lds > kMaxLds - 8 * 1024) return hipErrorInvalidValue;
  a.ld = padded_dim(a.d);
  a.ss = a.ld / 8 + 12;  // (as launch_sketch_tail)
  a.lds_words = (uint32_t)(lds / 4);
  if (q_stride < a.ld) return hipErrorInvalidValue;
  const bool l2 = a.metric == M_L2 || a.metric == M_L2SQ;
  if (!l2 && a.metric != M_COS && a.metric != M_IP && a.metric != M_NIP) return hipErrorInvalidValue;
  auto kernel = l2 ? sketch_tail_group_kernel<true> : sketch_tail_group_kernel<false>;
  hipError_t e = allow_lds(kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(ng), dim3(kTailThreads), lds, s, a, q_stride);
  return hipGetLastError();
}

uint32_t sketch_thresh_blocks(uint32_t lists, uint32_t kp) { return (lists * kp + kThreshSlots - 1) / kThreshSlots; }

// (the grids and the collect's slice: filled in here, for both launchers alike)
static bool sketch_spread_shape(SketchSpreadArgs &a, size_t *collect_lds) {
  if (a.lists == 0 || a.kp == 0 || a.k == 0 || a.k > a.kp || a.k > (uint32_t)kSpreadThreads || !a.lo_words || !a.hi_words || !a.pay ||
      !a.parts || !a.live || !a.sync || !a.rows || !a.count || !a.info)
    return false;
  a.thresh_blocks = sketch_thresh_blocks(a.lists, a.kp);
  a.collect_lists = std::max(kCollectLists, (a.lists + kCollectMaxBlocks - 1) / kCollectMaxBlocks);
  a.collect_blocks = (a.lists + a.collect_lists - 1) / a.collect_lists;
  *collect_lds = ((((size_t)a.thresh_blocks * a.k + 3) & ~(size_t)3) + (size_t)a.collect_lists * a.kp + a.collect_lists) * 4;
  return *collect_lds <= 48 * 1024;
}

hipError_t launch_sketch_thresh(SketchSpreadArgs a, hipStream_t s) {
  size_t lds = 0;
  if (!sketch_spread_shape(a, &lds)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sketch_thresh_kernel, dim3(a.thresh_blocks), dim3(kSpreadThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sketch_collect(SketchSpreadArgs a, hipStream_t s) {
  size_t lds = 0;
  if (!sketch_spread_shape(a, &lds)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sketch_collect_kernel, dim3(a.collect_blocks), dim3(kSpreadThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_sketch_refine(SketchRefineArgs a, hipStream_t s) {
  if (a.thresh_blocks == 0 || a.k == 0 || a.k > (uint32_t)kSpreadThreads || !a.parts || !a.slots || !a.live || !a.pay || !a.X || !a.q ||
      !a.kt_out || a.d == 0)
    return hipErrorInvalidValue;
  a.ld = padded_dim(a.d);
  a.ss = a.ld / 8 + 12;  // (K1's panel row: 4 * odd dwords, the eight tail products behind the sums)
  a.np4 = (a.thresh_blocks * a.k + 3u) & ~3u;
  size_t lds = ((size_t)2 * a.np4 + (size_t)a.k * a.ss) * 4;
  if (lds > 96 * 1024) {  // rows too long for the block: the kernel publishes the sketch's own Kt
    a.ss = 0;
    lds = (size_t)2 * a.np4 * 4;
    if (lds > 96 * 1024) return hipErrorInvalidValue;
  }
  hipError_t e = allow_lds(sketch_refine_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sketch_refine_kernel, dim3(1), dim3(kTailThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace vt

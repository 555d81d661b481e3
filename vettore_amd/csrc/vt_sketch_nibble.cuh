// vt_sketch_nibble.cuh -- the one skeleton of the nibble sketches (K1s, 6 bits; K1f, 5 bits; K1n, 4 bits: vt_sketch_nibble.hip
// holds a Plane policy per width, the kernels and the launchers; layout: vt_device.h, Sketch6ScanArgs; bounds: DESIGN 4.10):
// the row builder and the pass, each written once, and the small helpers the pass is made of.
#pragma once
#include "vt_rowscore.cuh"
#include "vt_sketch.cuh"

namespace vt {
namespace {

// What a width's bits decide: a row's elements are quantised to [-kQ, kQ]; the high four bits of each go to H-runs of 32
// elements (a signed nibble each), the kLowBits below them to L-runs of 32 kHPerL elements (a nibble holds the low bits of
// kHPerL elements, one of each H-run the L-run lies beside).  Four bits: one plane, no L-run.
template <int BITS>
struct NibbleWidth {
  static_assert(BITS == 4 || BITS == 5 || BITS == 6, "a nibble and up to two bits below it");
  static constexpr int kQ = (1 << (BITS - 1)) - 1;
  static constexpr int kLowBits = BITS - 4;
  static constexpr uint32_t kHPerL = kLowBits ? 4 / kLowBits : 1;  // H-runs beside one L-run (one plane: the builder's step)
  __device__ static uint32_t l_runs(uint32_t ld8) { return kLowBits ? ld8 / (32 * kHPerL) : 0u; }
};

// One wave per row, a lane per 32 kHPerL elements: quantise to [-kQ, kQ], write the H-runs and the L-run of those elements,
// then the row's {s, rho, nu} in the tile's metadata run and the column's bound.
template <class Plane>
__device__ __forceinline__ void nibble_row(const float *__restrict__ X, size_t stride, uint32_t row, bool have_row, uint32_t d,
                                           uint32_t ld8, unsigned char *__restrict__ img, unsigned long long *max_norm, int lane) {
  constexpr int kQ = Plane::kQ, kLowBits = Plane::kLowBits, kHPerL = (int)Plane::kHPerL;
  const float *src = X + (size_t)row * stride;
  float m = 0.0f;
  if (have_row)
    for (uint32_t i = lane; i < d; i += kWave) m = fmaxf(m, fabsf(src[i]));
  m = wave_max_f(m);
  float s = m / (float)kQ;
  float inv = (float)kQ / m;
  const bool quantise = have_row && m > 0.0f && finite_f32(inv) && s > 0.0f;
  if (!quantise) s = 0.0f;
  const uint32_t nh = ld8 / 32, nl = Plane::l_runs(ld8), runs = nh + nl + 1;
  double res = 0.0;   // sum of (x - s X)^2, f64
  uint32_t xx = 0;    // sum of X^2, exact
  for (uint32_t c = lane; c < nh / kHPerL; c += kWave) {
    uint32_t lw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int h = 0; h < kHPerL; ++h) {
      uint32_t hw[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const uint32_t i = (c * kHPerL + h) * 32 + j * 8 + b;
          const float x = have_row && i < d ? src[i] : 0.0f;
          int q = 0;
          if (quantise) {
            q = (int)rintf(x * inv);
            q = q > kQ ? kQ : (q < -kQ ? -kQ : q);
          }
          const double r = (double)x - (double)s * (double)q;  // (exact: s q has at most 24 + 5 significant bits)
          res += r * r;
          xx += (uint32_t)(q * q);
          word |= ((uint32_t)(q >> kLowBits) & 0xfu) << (4 * b);
          lw[j] |= ((uint32_t)q & ((1u << kLowBits) - 1u)) << (4 * b + kLowBits * h);
        }
        hw[j] = word;
      }
      *reinterpret_cast<u32x4 *>(img + sketch6_offset(row, kHPerL * c + h, runs)) = u32x4{hw[0], hw[1], hw[2], hw[3]};
    }
    if (kLowBits) *reinterpret_cast<u32x4 *>(img + sketch6_offset(row, nh + c, runs)) = u32x4{lw[0], lw[1], lw[2], lw[3]};
  }
  res = wave_sum_d(res);
  xx = wave_sum_u(xx);
  if (lane == 0) {
    const double rho = sqrt(res) * (1.0 + 0x1p-30);
    const double nu = (double)s * sqrt((double)xx) * (1.0 + 0x1p-30);
    const float rho_f = f32_up(rho), nu_f = f32_up(nu);
    *reinterpret_cast<u32x4 *>(img + sketch6_offset(row, nh + nl, runs)) =
        u32x4{__float_as_uint(s), __float_as_uint(rho_f), __float_as_uint(nu_f), 0u};
    const double bound = ((double)rho_f + (double)nu_f) * kSlack;
    atomicMax(max_norm, (unsigned long long)__double_as_longlong(bound));
  }
}

// The two builder kernels' bodies: every row of the image (rows past n_src as zero rows), or the listed rows in place.
template <class Plane>
__device__ __forceinline__ void nibble_build(const float *__restrict__ X, size_t stride, uint32_t n_src, uint32_t rows_img,
                                             uint32_t d, uint32_t ld8, unsigned char *img, unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= rows_img) return;
  nibble_row<Plane>(X, stride, w, w < n_src, d, ld8, img, max_norm, threadIdx.x & 63);
}
template <class Plane>
__device__ __forceinline__ void nibble_rows(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                            uint32_t count, uint32_t rows_img, uint32_t d, uint32_t ld8, unsigned char *img,
                                            unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= count) return;
  const uint32_t row = list[w];
  if (row >= rows_img) return;
  nibble_row<Plane>(X, stride, row, true, d, ld8, img, max_norm, threadIdx.x & 63);
}

typedef const __attribute__((address_space(4))) unsigned char *cq1_p;
typedef const __attribute__((address_space(4))) u32x4 *cq4_p;
// sixteen bytes of the query image, `off` bytes in (wave-uniform: one s_load_dwordx4)
__device__ __forceinline__ u32x4 qword(cq1_p img, uint32_t off) { return *(cq4_p)(img + off); }

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// dst = src / dst = 0 in the register dst already has
template <typename T, typename S>
__device__ __forceinline__ void park(T &dst, S src) {
  asm volatile("v_mov_b32 %0, %1" : "+v"(dst) : "v"(src));
}
template <typename T>
__device__ __forceinline__ void zero(T &dst) {
  asm volatile("v_mov_b32 %0, 0" : "+v"(dst));
}

__device__ __forceinline__ int dot8x4(const u32x4 x, const u32x4 q, int acc) {
  acc = __builtin_amdgcn_sdot8((int)x.x, (int)q.x, acc, false);
  acc = __builtin_amdgcn_sdot8((int)x.y, (int)q.y, acc, false);
  acc = __builtin_amdgcn_sdot8((int)x.z, (int)q.z, acc, false);
  acc = __builtin_amdgcn_sdot8((int)x.w, (int)q.w, acc, false);
  return acc;
}

__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, kWave);
    v = t < v ? t : v;
  }
  return v;
}

// K1n's threshold from each list's best rows (vt_device.h, Sketch6ScanArgs::best_words), by the wave that has
// just stored list `list`: tk holds the list's n entries, slot i with lane i (k <= kWave).  The two live slots of smallest
// key(lo) word, ties to the lower slot; the loads of both rows and of the query go out before any is waited for, three
// segments of 256 floats at a time; vt_rowscore.cuh does the rest.  S: 2 ss floats of LDS the wave owns -- its own buffer
// and that of the wave it absorbed, both done with: nothing of tk is read after the picks.
template <int CAP>
__device__ __forceinline__ void nibble_best_rows(const Sketch6ScanArgs &a, const WaveTopK<CAP> &tk, float *S, uint32_t list, int lane) {
  constexpr uint32_t kSegs = 3;
  const bool live = (uint32_t)lane < tk.n;
  const uint64_t p = live ? tk.bp[lane] : 0ull;
  const uint32_t w0 = live ? orderable(__uint_as_float((uint32_t)(p >> 32))) : 0xffffffffu;
  const uint32_t m0 = wave_min_u(w0);
  const int s0 = __ffsll((long long)__ballot(w0 == m0)) - 1;
  const uint32_t w1 = lane == s0 ? 0xffffffffu : w0;
  const uint32_t m1 = wave_min_u(w1);
  const int s1 = __ffsll((long long)__ballot(w1 == m1 && lane != s0)) - 1;
  const bool has0 = m0 != 0xffffffffu, has1 = m1 != 0xffffffffu;
  // (a slot that is not there: row 0, loaded and not used)
  const uint32_t r0 = has0 ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, s0) : 0u;
  const uint32_t r1 = has1 ? (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, s1) : 0u;
  wave_lds_fence();  // (the picks are read: the buffers are free)
  const uint32_t ld = padded_dim(a.d), ss = ld / 8 + 12, nseg = (ld + 255u) / 256u;
  const uint32_t cfull = a.d / 8, tail = a.d % 8, tail_base = ss - 12;
  const float *x0 = a.X + (size_t)r0 * a.stride, *x1 = a.X + (size_t)r1 * a.stride;
  const uint32_t l4 = (uint32_t)lane * 4u;
  const int odd = lane & 1;
  for (uint32_t g = 0; g < nseg; g += kSegs) {
    f32x4 v0[kSegs], v1[kSegs], qv[kSegs];
#pragma unroll
    for (uint32_t u = 0; u < kSegs; ++u) {  // (a lane past the row's end loads the row's last four floats: nothing is asked for conditionally)
      const uint32_t col = (g + u) * 256u + l4, colc = col < ld ? col : ld - 4u;
      v0[u] = *reinterpret_cast<const f32x4 *>(x0 + colc);
      v1[u] = *reinterpret_cast<const f32x4 *>(x1 + colc);
      qv[u] = *reinterpret_cast<const f32x4 *>(a.q + colc);
    }
#pragma unroll
    for (uint32_t u = 0; u < kSegs; ++u) {
      const uint32_t col = (g + u) * 256u + l4;
      row_chunk<-1>(S, qv[u], v0[u], col, ld, cfull, tail_base, a.order, odd);
      row_chunk<-1>(S + ss, qv[u], v1[u], col, ld, cfull, tail_base, a.order, odd);
    }
  }
  wave_lds_fence();
  if (lane < (int)kSketch4BestRows) {
    uint32_t word;
    const bool ok = row_rank_word(a.metric, row_chain(S + (uint32_t)lane * ss, cfull, tail, tail_base), &word);
    a.best_words[(size_t)list * kSketch4BestRows + lane] = (lane ? has1 : has0) && ok ? word : 0xffffffffu;
  }
}

// The pass: K1q's skeleton (a wave owns tiles wave, wave + waves, ...; a ring of kU one-KiB non-temporal loads that runs on
// across tiles; the metadata as the tile's last load; WaveTopK lists of (key(hi), id rank) with key(lo) beside them).
// What a run multiplies with is wave-uniform, so it never touches a vector register: the query's nibble levels are read
// through the scalar cache (constant address space => s_load_dwordx4; the blit that wrote them is earlier on the stream),
// the words the next run needs one slot ahead of it, and every dot takes its query dword from an SGPR.  An H-run is four
// v_dot8_i32_i4 per level; what an L-run is, the Plane says -- the third level never meets the L plane: its share of the
// dot is bounded instead, c3 and w3 of Sketch6ScanArgs.  Per level the H and L sums stay apart (exact:
// 8 * 7 * 32768 < 2^23) and meet in f64, in Plane::sum.
// Every cursor is wave-uniform, so the kind of a slot's run is a scalar branch and each arm works on its own sums in place.
// That holds only while the compiler leaves the three-way branch as written: the unit is built with the CFG structurizer
// told to skip wave-uniform regions (Makefile, EXTRA_vt_sketch_nibble), or the arms are laid out in a row, each behind a
// flag, every sum stays live across all three and is copied in each (about 400 v_mov_b32 per tile at d = 768).  No vector
// load is conditional (the comment above tile_index, vt_scan.cuh, says what one cost).
//
// A Plane (beside NibbleWidth's constants) supplies what the widths do not share:
//   Sums              the sums a lane keeps (h0, h1, h2: the H sums of the three levels) with their park() / zero()
//   Words, fetch()    the 16-byte query words a slot carries (a, b, c: word c of levels 1, 2, 3 for an H-run) and the loads
//                     of run nc's, at byte offsets chosen by scalar selects (a metadata run loads words it never uses)
//   kBlockMajor       how the waves are numbered: block by block, or across the blocks first
//   kBlockLists       the lists a block leaves
//   l_run()           an L-run's dots
//   sum()             how a finished tile's sums meet, in f64
//   gather()          the block's waves into its kBlockLists lists: whether the calling wave holds one to store
//   kBestRows         whether a storing wave may be asked for its list's best rows' exact keys (nibble_best_rows): a pair of
//                     waves a list, so that the wave owns two buffers once the list is stored
// Sums and Words are structs of named members, not arrays: as `int acc[3]` the sums cost the ring its order -- the eight loads
// ahead of the loop are issued last first, the first slot then waits for all of them (vmcnt(0), no wait in the other
// seven) and a group of eight runs behind its latest load (profiles/sketch_nibble/isa_counts.txt).
template <class Plane>
__device__ __forceinline__ void nibble_pass(const Sketch6ScanArgs &a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  static_assert(kSketch6Levels == 3, "levels 1-3 on the H plane, levels 1-2 on the L plane");
  const uint32_t nh = a.ld8 / 32, nl = Plane::l_runs(a.ld8);  // (nh: also the 16-byte words of one level of the query)
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *tkbuf = lds_raw + wib * WaveTopK<kCapSmall>::lds_bytes();

  WaveTopK<kCapSmall> tk;
  tk.init(tkbuf, a.k);
  const uint32_t ntiles = (a.n + kSketchTileRows - 1) / kSketchTileRows;
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  // (across the blocks first: neighbouring tiles go to different blocks, so a corpus of few tiles spreads over as many
  // lists as it has tiles, and a run of near-ties does not fill one list of 64 while the others stay empty; which tile
  // lands in which list is part of what a width's search returns on ties of the bounds, so each keeps its numbering)
  const uint32_t wave =
      uni(Plane::kBlockMajor ? blockIdx.x * kWavesPerBlock + wib : (uint32_t)wib * gridDim.x + blockIdx.x);
  const unsigned char *img = static_cast<const unsigned char *>(a.img);
  const uint32_t seg = nh + nl + 1;  // loads per tile (> kU: the launcher refuses ld8 = 128)

  if (wave < ntiles) {
    const uint32_t last_tile = wave + ((ntiles - 1 - wave) / waves) * waves;
    const uint32_t lane16 = (uint32_t)lane * 16;
    // the load cursor: run pc of tile pt, at `run`; past the wave's last tile it reads that tile again (never used)
    uint32_t pt = wave, pc = 0;
    const unsigned char *run = img + (size_t)wave * seg * 1024;
    const size_t next_tile = ((size_t)(waves - 1) * seg + 1) * 1024, same_tile = (size_t)(seg - 1) * 1024;
    auto load = [&]() -> u32x4 {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(run + lane16));
      if (pc + 1 == seg) {
        pc = 0;
        if (pt < last_tile) {
          pt += waves;
          run += next_tile;
        } else {
          run -= same_tile;
        }
      } else {
        pc += 1;
        run += 1024;
      }
      return v;
    };
    u32x4 buf[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) buf[u] = load();

    const cq1_p qimg = (cq1_p)(uintptr_t)a.qimg;  // [3][nh] words of 16 bytes
    const uint32_t level = uni(16 * nh);  // a level's bytes (opaque: 32 nc - 2 level must not fold into a VALU subtract-with-borrow)
    const double qn = a.qn, eta = a.eta, kerr = a.kerr;
    const double tiny = ((double)a.d + 16.0) * 0x1p-125;  // (K1's subnormal products, as in K1q)
    uint32_t ct = wave, cc = 0;  // compute cursor
    typename Plane::Sums acc;
    // a finished tile's sums and metadata, from the slot that met its last run to the end of the group (seg > kU: at most
    // one tile ends in a group); moved and zeroed with park() / zero(), which keep every value in the register it has
    typename Plane::Sums f;
    uint32_t ms = 0, mrho = 0, mnu = 0;
    // the operands of the run at cc
    typename Plane::Words q = Plane::fetch(qimg, 0, 1, 0, level);  // (run 0 is an H-run: with nh = 1 the selects fold)
    while (ct < ntiles) {
      // the groups up to the one the tile ends in: a loop of wave-uniform branches only; the tile's finish, divergent
      // code, follows it
      uint32_t fin = 0;
      const uint32_t ftile = ct;
      do {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const u32x4 x = buf[u];
          const bool isH = cc < nh, isL = cc < nh + nl;
          const uint32_t nc = uni(isL ? cc + 1 : 0u);  // the next run: its operands are on their way while this one works
          // (scalar loads return in any order, so a wait on them is a wait on all: this run's operands are waited for
          // here, before the next run's are asked for, and its dots then wait on no load issued in their own slot)
          __builtin_amdgcn_s_waitcnt(0xc07f);  // s_waitcnt lgkmcnt(0)
          const typename Plane::Words nq = Plane::fetch(qimg, nc, nh, nl, level);
          if (isH) {
            acc.h0 = dot8x4(x, q.a, acc.h0);
            acc.h1 = dot8x4(x, q.b, acc.h1);
            acc.h2 = dot8x4(x, q.c, acc.h2);
          } else if (isL) {
            Plane::l_run(acc, x, q, qimg, cc, level);
          } else {  // the tile's metadata: the rows are complete
            f.park(acc);
            park(ms, x.x);
            park(mrho, x.y);
            park(mnu, x.z);
            acc.zero();
            fin = 1;
            ct = uni(ct + waves);
          }
          // (the slot is refilled once its run is done with it: the load lands in the registers it frees, where a load
          // issued first needs eight more, copied back -- each behind a wait for its load -- at the head of every group)
          buf[u] = load();
          cc = nc;
          q = nq;
        }
      } while (!fin);
      const uint32_t row = ftile * kSketchTileRows + (uint32_t)lane;
      const bool valid = row < a.n;
      const double s = (double)__uint_as_float(ms);
      const double rho = (double)__uint_as_float(mrho), nu = (double)__uint_as_float(mnu);
      const double av = s * Plane::sum(a, f);
      double e = qn * rho + eta * nu + kerr * qn * (nu + rho) + 0x1p-40 * nu * (qn + eta);
      if (Plane::kLowBits) e += s * a.w3;  // (level 3's share on the L plane lies in c3 -+ w3)
      e = e * kSlack + tiny;
      const float hi = f32_up(av + e), lo = f32_down(av - e);
      float khi_rank, klo_rank;  // key(lo) >= key(hi): the rank functions fall as the dot rises
      if (a.metric == M_COS) {
        klo_rank = 1.0f - hi;
        khi_rank = 1.0f - lo;
      } else {
        klo_rank = -hi;
        khi_rank = -lo;
      }
      const uint32_t rank = valid ? (a.id_rank ? a.id_rank[row] : row) : 0u;
      const uint64_t key = ((uint64_t)orderable(klo_rank) << 32) | rank;
      tk.offer(valid, key, row, khi_rank, lane);
    }
  }
  __shared__ uint32_t s_counts[kWavesPerBlock];
  if (Plane::gather(tk, s_counts, wib, lane)) {
    // WaveTopK::store, and beside the list its two words per slot for the tail: orderable key(lo) and key(hi), an empty
    // slot 0xffffffff in both (no live entry is: the bounds are finite or infinite, never NaN)
    tk.compact(lane);
    const uint32_t list = Plane::kBlockLists > 1 ? (uint32_t)wib * Plane::kBlockLists / kWavesPerBlock : 0u;
    const size_t at = ((size_t)blockIdx.x * Plane::kBlockLists + list) * a.k;
    uint64_t *keys = a.part_keys + at;
    Payload *pay = a.part_pay + at;
    uint32_t *wlo = a.lo_words + at, *whi = a.hi_words + at;
    for (uint32_t i = lane; i < tk.k; i += kWave) {
      if (i < tk.n) {
        const uint64_t key = tk.bk[i], p = tk.bp[i];
        Payload pl;
        pl.row = (uint32_t)p;
        pl.raw = __uint_as_float((uint32_t)(p >> 32));
        keys[i] = key;
        pay[i] = pl;
        wlo[i] = orderable(pl.raw);
        whi[i] = (uint32_t)(key >> 32);
      } else {
        keys[i] = kEmptyKey;
        wlo[i] = 0xffffffffu;
        whi[i] = 0xffffffffu;
      }
    }
    if constexpr (Plane::kBestRows) {
      // (the storing wave's buffer and the one behind it, which it absorbed: no wave reads either again)
      if (a.best_words) nibble_best_rows(a, tk, reinterpret_cast<float *>(tkbuf), blockIdx.x * Plane::kBlockLists + list, lane);
    }
  }
}

}  // namespace
}  // namespace vt

// vt_sketch6.hip -- K1s's pass: a lone cosine / dot search nominated from the 6-bit sketch in two planes (gfx950; layout:
// vt_device.h, Sketch6ScanArgs; bounds: DESIGN 4.10).  The sketch's builders and the tail behind the pass are in vt_sketch.hip.
// A unit of its own because of how it is compiled: see the comment above the kernel and EXTRA_vt_sketch6 in the Makefile.
#include "vt_sketch.cuh"

namespace vt {

namespace {

// The pass: K1q's skeleton (a wave owns tiles wave, wave + waves, ...; a ring of kU one-KiB non-temporal loads that runs on
// across tiles; the metadata as the tile's last load; WaveTopK lists of (key(hi), id rank) with key(lo) beside them).
// What a run multiplies with is wave-uniform, so it never touches a vector register: the query's nibble levels are read
// through the scalar cache (constant address space => s_load_dwordx4; the blit that wrote them is earlier on the stream),
// the four words the next run needs one slot ahead of it, and every dot takes its query dword from an SGPR.  An H-run
// is four v_dot8_i32_i4 per level; an L-run, after four masks, four shifts and four masks, eight dots for each of the
// first two levels -- the third level never meets the L plane: its share of the dot is bounded instead, c3 and w3 of
// Sketch6ScanArgs.  Per level the H and L sums stay apart (exact: 8 * 7 * 32768 < 2^23) and meet in f64:
// a_r = s_r (sum_j t_j (4 accH_j + accL_j) + c3).
// Every cursor is wave-uniform, so the kind of a slot's run is a scalar branch and each arm works on its own sums in place.
// That holds only while the compiler leaves the three-way branch as written: this unit is built with the CFG structurizer
// told to skip wave-uniform regions (Makefile, EXTRA_vt_sketch6), or the arms are laid out in a row, each behind a flag,
// every sum stays live across all three and is copied in each (about 400 v_mov_b32 per tile at d = 768).  No vector load
// is conditional (the comment above tile_index, vt_scan.cuh, says what one cost).
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

__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch6_scan_kernel(const Sketch6ScanArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  static_assert(kSketch6Levels == 3, "levels 1-3 on the H plane, levels 1-2 on the L plane");
  const uint32_t nh = a.ld8 / 32, nl = a.ld8 / 64;  // (nh: also the 16-byte words of one level of the query)
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *tkbuf = lds_raw + wib * WaveTopK<kCapSmall>::lds_bytes();

  WaveTopK<kCapSmall> tk;
  tk.init(tkbuf, a.k);
  const uint32_t ntiles = (a.n + kSketchTileRows - 1) / kSketchTileRows;
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave = uni(blockIdx.x * kWavesPerBlock + wib);
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
    int aH0 = 0, aH1 = 0, aH2 = 0, aL0 = 0, aL1 = 0;
    // a finished tile's sums and metadata, from the slot that met its last run to the end of the group (seg > kU: at most
    // one tile ends in a group); moved and zeroed with park() / zero(), which keep every value in the register it has
    int fH0 = 0, fH1 = 0, fH2 = 0, fL0 = 0, fL1 = 0;
    uint32_t ms = 0, mrho = 0, mnu = 0;
    // The operands of the run at cc.  H-run c: word c of levels 1, 2, 3 in qa, qb, qc.  L-run c': words 2 c', 2 c' + 1 of
    // level 1 in qa, qb and of level 2 in qc, qd.  Always four loads, the offsets chosen by scalar selects: a metadata
    // run loads words it never uses.
    u32x4 qa = qword(qimg, 0), qb = qword(qimg, level), qc = qword(qimg, 2 * level), qd = qa;
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
          const bool nH = nc < nh;
          const uint32_t lb = nc < nh + nl ? 32 * nc - 2 * level : 0u;  // (an L-run's first word; nH: not used)
          const uint32_t oa = nH ? 16 * nc : lb;
          // (scalar loads return in any order, so a wait on them is a wait on all: this run's operands are waited for
          // here, before the next run's are asked for, and its dots then wait on no load issued in their own slot)
          __builtin_amdgcn_s_waitcnt(0xc07f);  // s_waitcnt lgkmcnt(0)
          const u32x4 na = qword(qimg, oa), nb = qword(qimg, oa + (nH ? level : 16u));
          const u32x4 nq = qword(qimg, oa + (nH ? 2 * level : level)), nd = qword(qimg, oa + (nH ? 0u : level + 16u));
          if (isH) {
            aH0 = dot8x4(x, qa, aH0);
            aH1 = dot8x4(x, qb, aH1);
            aH2 = dot8x4(x, qc, aH2);
          } else if (isL) {
            const u32x4 lo = x & 0x33333333u, hi = (x >> 2) & 0x33333333u;
            aL0 = dot8x4(lo, qa, aL0);
            aL0 = dot8x4(hi, qb, aL0);
            aL1 = dot8x4(lo, qc, aL1);
            aL1 = dot8x4(hi, qd, aL1);
          } else {  // the tile's metadata: the rows are complete
            park(fH0, aH0);
            park(fH1, aH1);
            park(fH2, aH2);
            park(fL0, aL0);
            park(fL1, aL1);
            park(ms, x.x);
            park(mrho, x.y);
            park(mnu, x.z);
            zero(aH0);
            zero(aH1);
            zero(aH2);
            zero(aL0);
            zero(aL1);
            fin = 1;
            ct = uni(ct + waves);
          }
          // (the slot is refilled once its run is done with it: the load lands in the registers it frees, where a load
          // issued first needs eight more, copied back -- each behind a wait for its load -- at the head of every group)
          buf[u] = load();
          cc = nc;
          qa = na;
          qb = nb;
          qc = nq;
          qd = nd;
        }
      } while (!fin);
      const uint32_t row = ftile * kSketchTileRows + (uint32_t)lane;
      const bool valid = row < a.n;
      const double s = (double)__uint_as_float(ms);
      const double rho = (double)__uint_as_float(mrho), nu = (double)__uint_as_float(mnu);
      // (each product exact; level 3's share on the L plane lies in c3 -+ w3)
      const double sum = (double)a.t[0] * (double)(4 * fH0 + fL0) + (double)a.t[1] * (double)(4 * fH1 + fL1) +
                         (double)a.t[2] * (double)(4 * fH2) + a.c3;
      const double av = s * sum;
      const double e =
          (qn * rho + eta * nu + kerr * qn * (nu + rho) + 0x1p-40 * nu * (qn + eta) + s * a.w3) * kSlack + tiny;
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
  tk.merge_block(wib, kWavesPerBlock, s_counts, lane);
  if (wib == 0) {
    // WaveTopK::store, and beside the list its two words per slot for the tail: orderable key(lo) and key(hi), an empty
    // slot 0xffffffff in both (no live entry is: the bounds are finite or infinite, never NaN)
    tk.compact(lane);
    uint64_t *keys = a.part_keys + (size_t)blockIdx.x * a.k;
    Payload *pay = a.part_pay + (size_t)blockIdx.x * a.k;
    uint32_t *wlo = a.lo_words + (size_t)blockIdx.x * a.k, *whi = a.hi_words + (size_t)blockIdx.x * a.k;
    for (uint32_t i = lane; i < tk.k; i += kWave) {
      if (i < tk.n) {
        const uint64_t key = tk.bk[i], p = tk.bp[i];
        Payload q;
        q.row = (uint32_t)p;
        q.raw = __uint_as_float((uint32_t)(p >> 32));
        keys[i] = key;
        pay[i] = q;
        wlo[i] = orderable(q.raw);
        whi[i] = (uint32_t)(key >> 32);
      } else {
        keys[i] = kEmptyKey;
        wlo[i] = 0xffffffffu;
        whi[i] = 0xffffffffu;
      }
    }
  }
}

}  // namespace

size_t sketch6_scan_lds_bytes(uint32_t d, uint32_t k) {
  if (d == 0 || d > kSketchMaxDim || k == 0 || k > (uint32_t)kSmallK) return 0;
  if (sketch6_runs(d) <= (uint32_t)kU) return 0;  // (ld8 = 128: two tiles could end in one group of loads)
  return kWavesPerBlock * WaveTopK<kCapSmall>::lds_bytes();  // (the list buffers: the query comes through the scalar cache)
}

hipError_t launch_sketch6_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = sketch6_scan_lds_bytes(a.d, a.k);
  if (!lds || a.ld8 != sketch_ld8(a.d) || blocks == 0 || !a.part_keys || !a.part_pay || !a.lo_words || !a.hi_words)
    return hipErrorInvalidValue;
  hipError_t e = allow_lds(sketch6_scan_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sketch6_scan_kernel, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace vt

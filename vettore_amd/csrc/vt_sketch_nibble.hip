// vt_sketch_nibble.hip -- K1s, K1f and K1n: a lone cosine / dot search nominated from the 6-bit or 5-bit sketch in two planes
// or from the 4-bit sketch in one (gfx950; layout: vt_device.h, Sketch6ScanArgs and above launch_sketch5_scan /
// launch_sketch4_scan; bounds and K1n's exact threshold behind the pass: DESIGN 4.10).  The builders and the pass are written
// once, in vt_sketch_nibble.cuh; here are the three widths' Plane policies, the kernels and their launchers.  The tail, the
// threshold, refine and collect kernels behind the passes are in vt_sketch.hip.
// A unit of its own because of how it is compiled: see the comment above nibble_pass and EXTRA_vt_sketch_nibble in the Makefile.
#include "vt_sketch_nibble.cuh"

namespace vt {

namespace {

// K1s and K1f: an H plane and an L plane.  The operands of the run at cc -- H-run c: word c of levels 1, 2, 3 in q.a, q.b,
// q.c.  L-run c': words kHPerL c', kHPerL c' + 1 of level 1 in q.a, q.b and of level 2 in q.c, q.d.  Always four
// loads, the offsets chosen by scalar selects.  a_r = s_r (sum_j t_j (2^kLowBits accH_j + accL_j) + c3).  One list a block.
template <int BITS>
struct TwoPlanes : NibbleWidth<BITS> {
  using W = NibbleWidth<BITS>;
  struct Sums {  // H of levels 1-3, L of levels 1-2
    int h0 = 0, h1 = 0, h2 = 0, l0 = 0, l1 = 0;
    __device__ __forceinline__ void park(const Sums &a) {
      vt::park(h0, a.h0);
      vt::park(h1, a.h1);
      vt::park(h2, a.h2);
      vt::park(l0, a.l0);
      vt::park(l1, a.l1);
    }
    __device__ __forceinline__ void zero() {
      vt::zero(h0);
      vt::zero(h1);
      vt::zero(h2);
      vt::zero(l0);
      vt::zero(l1);
    }
  };
  static constexpr uint32_t kBlockLists = 1;
  static constexpr bool kBestRows = false;
  struct Words {
    u32x4 a, b, c, d;
  };
  __device__ __forceinline__ static Words fetch(cq1_p qimg, uint32_t nc, uint32_t nh, uint32_t nl, uint32_t level) {
    const bool nH = nc < nh;
    const uint32_t lb = nc < nh + nl ? 16 * W::kHPerL * nc - W::kHPerL * level : 0u;  // (an L-run's first word; nH: not used)
    const uint32_t oa = nH ? 16 * nc : lb;
    // (opaque, as level is: a select between level and a 2 level of no other use folds into a shift by the flag, on the VALU)
    const uint32_t level2 = uni(2 * level);
    return Words{qword(qimg, oa), qword(qimg, oa + (nH ? level : 16u)), qword(qimg, oa + (nH ? level2 : level)),
                 qword(qimg, oa + (nH ? 0u : level + 16u))};
  }
  __device__ __forceinline__ static double sum(const Sketch6ScanArgs &a, const Sums &f) {
    constexpr int kH = 1 << W::kLowBits;  // (each product exact; level 3's share on the L plane lies in c3 -+ w3)
    return (double)a.t[0] * (double)(kH * f.h0 + f.l0) + (double)a.t[1] * (double)(kH * f.h1 + f.l1) +
           (double)a.t[2] * (double)(kH * f.h2) + a.c3;
  }
  __device__ __forceinline__ static bool gather(WaveTopK<kCapSmall> &tk, uint32_t *counts, int wib, int lane) {
    tk.merge_block(wib, kWavesPerBlock, counts, lane);
    return wib == 0;
  }
};

// K1s: an L-run holds two bits of 64 elements -- four masks, four shifts and four masks, then eight dots for each of the
// first two levels.  The waves are numbered block by block.
struct Plane6 : TwoPlanes<6> {
  static constexpr bool kBlockMajor = true;
  __device__ __forceinline__ static void l_run(Sums &acc, const u32x4 x, const Words &q, cq1_p, uint32_t, uint32_t) {
    const u32x4 lo = x & 0x33333333u, hi = (x >> 2) & 0x33333333u;
    acc.l0 = dot8x4(lo, q.a, acc.l0);
    acc.l0 = dot8x4(hi, q.b, acc.l0);
    acc.l1 = dot8x4(lo, q.c, acc.l1);
    acc.l1 = dot8x4(hi, q.d, acc.l1);
  }
};

// K1f: an L-run holds one bit of 128 elements: four shifts and masks give the nibble vectors of four H-runs, dotted with
// levels 1 and 2 -- eight query words where a slot carries four, so the run is walked in two halves: the first on the words
// the slot before asked for (H-runs 4 c', 4 c' + 1), the second (4 c' + 2, 4 c' + 3) on four more asked for at the arm's
// head, behind a wait of its own.
struct Plane5 : TwoPlanes<5> {
  static constexpr bool kBlockMajor = false;
  __device__ __forceinline__ static void l_run(Sums &acc, const u32x4 x, const Words &q, cq1_p qimg, uint32_t cc,
                                               uint32_t level) {
    const uint32_t hb = uni(64 * cc - 4 * level + 32);
    const u32x4 ra = qword(qimg, hb), rb = qword(qimg, hb + 16u);
    const u32x4 rc = qword(qimg, hb + level), rd = qword(qimg, hb + level + 16u);
    const u32x4 v0 = x & 0x11111111u, v1 = (x >> 1) & 0x11111111u;
    acc.l0 = dot8x4(v0, q.a, acc.l0);
    acc.l0 = dot8x4(v1, q.b, acc.l0);
    acc.l1 = dot8x4(v0, q.c, acc.l1);
    acc.l1 = dot8x4(v1, q.d, acc.l1);
    const u32x4 v2 = (x >> 2) & 0x11111111u, v3 = (x >> 3) & 0x11111111u;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // (the next run's words with them)
    acc.l0 = dot8x4(v2, ra, acc.l0);
    acc.l0 = dot8x4(v3, rb, acc.l0);
    acc.l1 = dot8x4(v2, rc, acc.l1);
    acc.l1 = dot8x4(v3, rd, acc.l1);
  }
};

// K1n: one plane of signed nibbles with a scale of its own, s = max|x| / 7 -- H-runs and nothing else: no L plane, no
// c3 / w3, no load issued and awaited inside a slot.  a_r = s_r sum_j t_j acc_j.  Each block leaves TWO lists (waves 0-1,
// waves 2-3): the intervals are twice K1f's, and the candidates behind the exact threshold (vt_sketch.hip,
// sketch_refine_kernel) number what K1f's do behind the sketch's own -- with a wider spread, hence twice the slots.
// The pair's storing wave may be asked for the exact keys of the list's two best rows (kBestRows; nibble_best_rows): the
// threshold then needs no launch of its own.
struct Plane4 : NibbleWidth<4> {
  struct Sums {
    int h0 = 0, h1 = 0, h2 = 0;
    __device__ __forceinline__ void park(const Sums &a) {
      vt::park(h0, a.h0);
      vt::park(h1, a.h1);
      vt::park(h2, a.h2);
    }
    __device__ __forceinline__ void zero() {
      vt::zero(h0);
      vt::zero(h1);
      vt::zero(h2);
    }
  };
  static constexpr bool kBlockMajor = false;
  static constexpr uint32_t kBlockLists = kSketch4BlockLists;
  static constexpr bool kBestRows = true;
  static_assert(kWavesPerBlock == 2 * (int)kSketch4BlockLists, "a list per pair of waves");
  static_assert(kSketch4BestRows * kSketch4BestRowFloats * sizeof(float) <= 2 * WaveTopK<kCapSmall>::lds_bytes(),
                "the best rows' chunk sums lie in the pair's two wave buffers");
  struct Words {
    u32x4 a, b, c;
  };
  __device__ __forceinline__ static Words fetch(cq1_p qimg, uint32_t nc, uint32_t nh, uint32_t, uint32_t level) {
    const uint32_t oa = nc < nh ? 16 * nc : 0u;  // (the metadata run next: word 0 again, in bounds and never used)
    return Words{qword(qimg, oa), qword(qimg, oa + level), qword(qimg, oa + 2 * level)};
  }
  __device__ __forceinline__ static void l_run(Sums &, const u32x4, const Words &, cq1_p, uint32_t, uint32_t) {}
  __device__ __forceinline__ static double sum(const Sketch6ScanArgs &a, const Sums &f) {
    return (double)a.t[0] * (double)f.h0 + (double)a.t[1] * (double)f.h1 + (double)a.t[2] * (double)f.h2;
  }
  // an even wave takes in the buffer of the wave behind it (the buffers lie wave by wave in LDS)
  __device__ __forceinline__ static bool gather(WaveTopK<kCapSmall> &tk, uint32_t *counts, int wib, int lane) {
    tk.compact(lane);
    if (lane == 0) counts[wib] = tk.n;
    __syncthreads();
    if (wib & 1) return false;
    tk.absorb(tk.bk + 2 * kCapSmall, counts[wib + 1], lane);
    return true;
  }
};

// The kernels: a width's policy into the shared bodies.
__global__ __launch_bounds__(256) void sketch6_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                            uint32_t rows_img, uint32_t d, uint32_t ld8, unsigned char *img,
                                                            unsigned long long *max_norm) {
  nibble_build<Plane6>(X, stride, n_src, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(256) void sketch6_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                           uint32_t count, uint32_t rows_img, uint32_t d, uint32_t ld8,
                                                           unsigned char *img, unsigned long long *max_norm) {
  nibble_rows<Plane6>(X, stride, list, count, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(256) void sketch5_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                            uint32_t rows_img, uint32_t d, uint32_t ld8, unsigned char *img,
                                                            unsigned long long *max_norm) {
  nibble_build<Plane5>(X, stride, n_src, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(256) void sketch5_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                           uint32_t count, uint32_t rows_img, uint32_t d, uint32_t ld8,
                                                           unsigned char *img, unsigned long long *max_norm) {
  nibble_rows<Plane5>(X, stride, list, count, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(256) void sketch4_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                            uint32_t rows_img, uint32_t d, uint32_t ld8, unsigned char *img,
                                                            unsigned long long *max_norm) {
  nibble_build<Plane4>(X, stride, n_src, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(256) void sketch4_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                           uint32_t count, uint32_t rows_img, uint32_t d, uint32_t ld8,
                                                           unsigned char *img, unsigned long long *max_norm) {
  nibble_rows<Plane4>(X, stride, list, count, rows_img, d, ld8, img, max_norm);
}
__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch6_scan_kernel(const Sketch6ScanArgs a) { nibble_pass<Plane6>(a); }
__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch5_scan_kernel(const Sketch6ScanArgs a) { nibble_pass<Plane5>(a); }
__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch4_scan_kernel(const Sketch6ScanArgs a) { nibble_pass<Plane4>(a); }

// The launchers' bodies, once: the kernel and the width's runs per tile are what a width's launcher adds.
template <class K>
hipError_t nibble_launch_build(K kernel, const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                               unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim || rows_img % kSketchTileRows) return hipErrorInvalidValue;
  if (rows_img == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3((rows_img + 3) / 4), dim3(256), 0, s, X, stride, n_src, rows_img, d, sketch_ld8(d),
                     static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

template <class K>
hipError_t nibble_launch_rows(K kernel, const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img,
                              uint32_t d, void *img, unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3((count + 3) / 4), dim3(256), 0, s, X, stride, list, count, rows_img, d, sketch_ld8(d),
                     static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

size_t nibble_scan_lds_bytes(uint32_t runs, uint32_t d, uint32_t k) {
  if (d == 0 || d > kSketchMaxDim || k == 0 || k > (uint32_t)kSmallK) return 0;
  if (runs <= (uint32_t)kU) return 0;  // (ld8 = 128: two tiles could end in one group of loads)
  return kWavesPerBlock * WaveTopK<kCapSmall>::lds_bytes();  // (the list buffers: the query comes through the scalar cache)
}

// (best_rows: the width's pass takes Sketch6ScanArgs::best_words)
template <class K>
hipError_t nibble_launch_scan(K kernel, size_t lds, bool best_rows, const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s) {
  if (!lds || a.ld8 != sketch_ld8(a.d) || blocks == 0 || !a.part_keys || !a.part_pay || !a.lo_words || !a.hi_words)
    return hipErrorInvalidValue;
  if (a.best_words && (!best_rows || !a.X || !a.q || a.stride < padded_dim(a.d) || a.k > (uint32_t)kWave ||
                       padded_dim(a.d) / 8 + 12 > kSketch4BestRowFloats ||
                       (a.metric != M_COS && a.metric != M_IP && a.metric != M_NIP)))
    return hipErrorInvalidValue;
  hipError_t e = allow_lds(kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace

// (vt_device.h declares these four per width)
#define VT_NIBBLE_LAUNCHERS(N)                                                                                                     \
  hipError_t launch_sketch##N##_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,     \
                                      unsigned long long *max_norm, hipStream_t s) {                                               \
    return nibble_launch_build(sketch##N##_build_kernel, X, stride, n_src, rows_img, d, img, max_norm, s);                         \
  }                                                                                                                                \
  hipError_t launch_sketch##N##_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img,       \
                                     uint32_t d, void *img, unsigned long long *max_norm, hipStream_t s) {                         \
    return nibble_launch_rows(sketch##N##_rows_kernel, X, stride, list, count, rows_img, d, img, max_norm, s);                     \
  }                                                                                                                                \
  size_t sketch##N##_scan_lds_bytes(uint32_t d, uint32_t k) { return nibble_scan_lds_bytes(sketch##N##_runs(d), d, k); }           \
  hipError_t launch_sketch##N##_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s) {                                   \
    return nibble_launch_scan(sketch##N##_scan_kernel, sketch##N##_scan_lds_bytes(a.d, a.k), N == 4, a, blocks, s);                \
  }
VT_NIBBLE_LAUNCHERS(6)
VT_NIBBLE_LAUNCHERS(5)
VT_NIBBLE_LAUNCHERS(4)

}  // namespace vt

// vt_sketch4.hip -- K1n: a lone cosine / dot search nominated from the 4-bit sketch (gfx950; layout: vt_device.h above
// launch_sketch4_scan; bounds and the exact threshold behind the pass: DESIGN 4.10), its builders and its pass.  The column
// is one plane of signed nibbles with a scale of its own, s = max|x| / 7: K1s's H-runs and nothing else, so the pass is
// K1s's loop with one kind of data run -- no L plane, no c3 / w3, no load issued and awaited inside a slot.  Compiled like
// vt_sketch6.hip (EXTRA_vt_sketch4 in the Makefile).  Each block leaves TWO lists (waves 0-1, waves 2-3): the intervals
// are twice K1f's, and the candidates behind the exact threshold (vt_sketch.hip, sketch_refine_kernel) number what K1f's
// do behind the sketch's own -- with a wider spread, hence twice the slots.
#include "vt_sketch.cuh"

namespace vt {

namespace {

// One wave per row, a lane per 32 elements: quantise to [-7, 7], write the H-run of those elements.
__device__ __forceinline__ void sketch4_row(const float *__restrict__ X, size_t stride, uint32_t row, bool have_row, uint32_t d,
                                            uint32_t ld8, unsigned char *__restrict__ img, unsigned long long *max_norm, int lane) {
  const float *src = X + (size_t)row * stride;
  float m = 0.0f;
  if (have_row)
    for (uint32_t i = lane; i < d; i += kWave) m = fmaxf(m, fabsf(src[i]));
  m = wave_max_f(m);
  float s = m / 7.0f;
  float inv = 7.0f / m;
  const bool quantise = have_row && m > 0.0f && finite_f32(inv) && s > 0.0f;
  if (!quantise) s = 0.0f;
  const uint32_t nh = ld8 / 32, runs = nh + 1;
  double res = 0.0;   // sum of (x - s X)^2, f64
  uint32_t xx = 0;    // sum of X^2, exact
  for (uint32_t c = lane; c < nh; c += kWave) {
    uint32_t hw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const uint32_t i = c * 32 + j * 8 + b;
        const float x = have_row && i < d ? src[i] : 0.0f;
        int q = 0;
        if (quantise) {
          q = (int)rintf(x * inv);
          q = q > 7 ? 7 : (q < -7 ? -7 : q);
        }
        const double r = (double)x - (double)s * (double)q;  // (exact: s q has at most 27 significant bits)
        res += r * r;
        xx += (uint32_t)(q * q);
        word |= ((uint32_t)q & 0xfu) << (4 * b);
      }
      hw[j] = word;
    }
    *reinterpret_cast<u32x4 *>(img + sketch6_offset(row, c, runs)) = u32x4{hw[0], hw[1], hw[2], hw[3]};
  }
  res = wave_sum_d(res);
  xx = wave_sum_u(xx);
  if (lane == 0) {
    const double rho = sqrt(res) * (1.0 + 0x1p-30);
    const double nu = (double)s * sqrt((double)xx) * (1.0 + 0x1p-30);
    const float rho_f = f32_up(rho), nu_f = f32_up(nu);
    *reinterpret_cast<u32x4 *>(img + sketch6_offset(row, nh, runs)) =
        u32x4{__float_as_uint(s), __float_as_uint(rho_f), __float_as_uint(nu_f), 0u};
    const double bound = ((double)rho_f + (double)nu_f) * kSlack;
    atomicMax(max_norm, (unsigned long long)__double_as_longlong(bound));
  }
}

__global__ __launch_bounds__(256) void sketch4_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                            uint32_t rows_img, uint32_t d, uint32_t ld8, unsigned char *img,
                                                            unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= rows_img) return;
  sketch4_row(X, stride, w, w < n_src, d, ld8, img, max_norm, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void sketch4_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                           uint32_t count, uint32_t rows_img, uint32_t d, uint32_t ld8,
                                                           unsigned char *img, unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= count) return;
  const uint32_t row = list[w];
  if (row >= rows_img) return;
  sketch4_row(X, stride, row, true, d, ld8, img, max_norm, threadIdx.x & 63);
}

// The pass: sketch6_scan_kernel's skeleton (vt_sketch6.hip says why each piece is as it is: a wave owns tiles wave,
// wave + waves, ... with the waves numbered block by block; a ring of kU one-KiB non-temporal loads that runs on across
// tiles; the metadata as the tile's last load; the query's nibble levels through the scalar cache, the next run's three
// words one slot ahead, behind the explicit wait; wave-uniform cursors, the kind of a slot's run a scalar branch; the
// tile's finish outside the loop of uniform branches).  Every data run is an H-run: four v_dot8_i32_i4 per level, twelve a
// run.  a_r = s_r sum_j t_j acc_j, each product exact in f64.
typedef const __attribute__((address_space(4))) unsigned char *cq1_p;
typedef const __attribute__((address_space(4))) u32x4 *cq4_p;
__device__ __forceinline__ u32x4 qword(cq1_p img, uint32_t off) { return *(cq4_p)(img + off); }

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

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

__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch4_scan_kernel(const Sketch6ScanArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  static_assert(kSketch6Levels == 3, "three levels on the one plane");
  static_assert(kWavesPerBlock == 2 * (int)kSketch4BlockLists, "a list per pair of waves");
  const uint32_t nh = a.ld8 / 32;  // (also the 16-byte words of one level of the query)
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char *tkbuf = lds_raw + wib * WaveTopK<kCapSmall>::lds_bytes();

  WaveTopK<kCapSmall> tk;
  tk.init(tkbuf, a.k);
  const uint32_t ntiles = (a.n + kSketchTileRows - 1) / kSketchTileRows;
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave = uni((uint32_t)wib * gridDim.x + blockIdx.x);
  const unsigned char *img = static_cast<const unsigned char *>(a.img);
  const uint32_t seg = nh + 1;  // loads per tile (> kU: the launcher refuses ld8 = 128)

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
    const uint32_t level = uni(16 * nh);  // a level's bytes (opaque, as in K1s's pass)
    const double qn = a.qn, eta = a.eta, kerr = a.kerr;
    const double tiny = ((double)a.d + 16.0) * 0x1p-125;  // (K1's subnormal products, as in K1q)
    uint32_t ct = wave, cc = 0;  // compute cursor
    int a0 = 0, a1 = 0, a2 = 0;
    // a finished tile's sums and metadata, from the slot that met its last run to the end of the group (seg > kU: at most
    // one tile ends in a group)
    int f0 = 0, f1 = 0, f2 = 0;
    uint32_t ms = 0, mrho = 0, mnu = 0;
    // the operands of the run at cc: word cc of levels 1, 2, 3 (a metadata run loads words it never uses)
    u32x4 qa = qword(qimg, 0), qb = qword(qimg, level), qc = qword(qimg, 2 * level);
    while (ct < ntiles) {
      uint32_t fin = 0;
      const uint32_t ftile = ct;
      do {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const u32x4 x = buf[u];
          const bool isH = cc < nh;
          const uint32_t nc = uni(isH ? cc + 1 : 0u);  // the next run: its operands are on their way while this one works
          const uint32_t oa = nc < nh ? 16 * nc : 0u;  // (the metadata run next: word 0 again, in bounds and never used)
          __builtin_amdgcn_s_waitcnt(0xc07f);  // s_waitcnt lgkmcnt(0): this run's operands
          const u32x4 na = qword(qimg, oa), nb = qword(qimg, oa + level), nq = qword(qimg, oa + 2 * level);
          if (isH) {
            a0 = dot8x4(x, qa, a0);
            a1 = dot8x4(x, qb, a1);
            a2 = dot8x4(x, qc, a2);
          } else {  // the tile's metadata: the rows are complete
            park(f0, a0);
            park(f1, a1);
            park(f2, a2);
            park(ms, x.x);
            park(mrho, x.y);
            park(mnu, x.z);
            zero(a0);
            zero(a1);
            zero(a2);
            fin = 1;
            ct = uni(ct + waves);
          }
          buf[u] = load();
          cc = nc;
          qa = na;
          qb = nb;
          qc = nq;
        }
      } while (!fin);
      const uint32_t row = ftile * kSketchTileRows + (uint32_t)lane;
      const bool valid = row < a.n;
      const double s = (double)__uint_as_float(ms);
      const double rho = (double)__uint_as_float(mrho), nu = (double)__uint_as_float(mnu);
      const double sum = (double)a.t[0] * (double)f0 + (double)a.t[1] * (double)f1 + (double)a.t[2] * (double)f2;
      const double av = s * sum;
      const double e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 0x1p-40 * nu * (qn + eta)) * kSlack + tiny;
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
  // two lists a block: an even wave takes in the buffer of the wave behind it (the buffers lie wave by wave in LDS)
  __shared__ uint32_t s_counts[kWavesPerBlock];
  tk.compact(lane);
  if (lane == 0) s_counts[wib] = tk.n;
  __syncthreads();
  if ((wib & 1) == 0) {
    tk.absorb(tk.bk + 2 * kCapSmall, s_counts[wib + 1], lane);
    // the list and beside it its two words per slot for the tail, as sketch6_scan_kernel leaves them
    tk.compact(lane);
    const size_t at = ((size_t)blockIdx.x * kSketch4BlockLists + (uint32_t)(wib >> 1)) * a.k;
    uint64_t *keys = a.part_keys + at;
    Payload *pay = a.part_pay + at;
    uint32_t *wlo = a.lo_words + at, *whi = a.hi_words + at;
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

hipError_t launch_sketch4_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                                unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim || rows_img % kSketchTileRows) return hipErrorInvalidValue;
  if (rows_img == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch4_build_kernel, dim3((rows_img + 3) / 4), dim3(256), 0, s, X, stride, n_src, rows_img, d,
                     sketch_ld8(d), static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

hipError_t launch_sketch4_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                               void *img, unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch4_rows_kernel, dim3((count + 3) / 4), dim3(256), 0, s, X, stride, list, count, rows_img, d,
                     sketch_ld8(d), static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

size_t sketch4_scan_lds_bytes(uint32_t d, uint32_t k) {
  if (d == 0 || d > kSketchMaxDim || k == 0 || k > (uint32_t)kSmallK) return 0;
  if (sketch4_runs(d) <= (uint32_t)kU) return 0;  // (ld8 = 128: two tiles could end in one group of loads)
  return kWavesPerBlock * WaveTopK<kCapSmall>::lds_bytes();  // (the list buffers: the query comes through the scalar cache)
}

hipError_t launch_sketch4_scan(const Sketch6ScanArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = sketch4_scan_lds_bytes(a.d, a.k);
  if (!lds || a.ld8 != sketch_ld8(a.d) || blocks == 0 || !a.part_keys || !a.part_pay || !a.lo_words || !a.hi_words)
    return hipErrorInvalidValue;
  hipError_t e = allow_lds(sketch4_scan_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sketch4_scan_kernel, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

}  // namespace vt

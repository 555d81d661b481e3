// vt_sketch.hip -- K1q: a lone cosine / dot search nominated from an int8 sketch of the rows (gfx950).
//
// The sketch (layout and bounds: vt_device.h, SketchScanArgs) holds a quarter of the f32 rows' bytes.  K1q streams it
// once and gives every row an interval [lo_r, hi_r] that provably holds what K1 would compute for it:
//   * the query arrives as two int8 levels, q ~ t1 Q1 + t2 Q2; v_dot4c_i32_i8 forms Q1.X_r and Q2.X_r exactly in int32;
//   * a_r = s_r (t1 Q1.X_r + t2 Q2.X_r) in f64, e_r = ||q|| rho_r + ||eta|| nu_r + K1's summation error + f64 slack;
//     [a_r - e_r, a_r + e_r] is rounded outwards to f32;
//   * the rank function of the three metrics is monotone non-increasing in the dot, so key(hi_r) <= key_r <= key(lo_r):
//     every block keeps its k' smallest (key(hi_r), id rank) keys (WaveTopK, K1's list layout) with key(lo_r) beside them.
// sketch_certify_kernel then proves that the retained rows with key(hi) <= Kt hold the exact top k, and the gathered K1
// (exact arithmetic) rescores only those.
#include "vt_scan.cuh"

namespace vt {

using namespace dev;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, kWave);
  return v;
}

// f64 -> f32 rounded towards +inf / -inf (finite inputs)
__device__ __forceinline__ float f32_up(double v) {
  const float f = (float)v;
  return (double)f < v ? nextafterf(f, INFINITY) : f;
}
__device__ __forceinline__ float f32_down(double v) {
  const float f = (float)v;
  return (double)f > v ? nextafterf(f, -INFINITY) : f;
}
constexpr double kSlack = 1.0 + 0x1p-40;  // covers the f64 rounding of the bound's own arithmetic

// One wave per row: quantise, write the row's chunks and its {s, rho, nu} in the tiled layout.
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
        xx += (uint32_t)(q * q);
        word |= ((uint32_t)q & 0xffu) << (8 * b);
      }
      w[j] = word;
    }
    *reinterpret_cast<u32x4 *>(img + sketch_offset(row, c, nch)) = u32x4{w[0], w[1], w[2], w[3]};
  }
  res = wave_sum_d(res);
  xx = wave_sum_u(xx);
  if (lane == 0) {
    // (each f64 sum above carries at most d relative roundings of 2^-53: the 2^-30 margin covers any d this path takes)
    const double rho = sqrt(res) * (1.0 + 0x1p-30);
    const double nu = (double)s * sqrt((double)xx) * (1.0 + 0x1p-30);
    const float rho_f = f32_up(rho), nu_f = f32_up(nu);
    *reinterpret_cast<u32x4 *>(img + sketch_offset(row, nch, nch)) =
        u32x4{__float_as_uint(s), __float_as_uint(rho_f), __float_as_uint(nu_f), 0u};
    const double bound = ((double)rho_f + (double)nu_f) * kSlack;
    unsigned long long bits = (unsigned long long)__double_as_longlong(bound);
    atomicMax(max_norm, bits);  // (non-negative f64: the bit patterns order like the values)
  }
}

__global__ __launch_bounds__(256) void sketch_build_kernel(const float *__restrict__ X, size_t stride, uint32_t n_src,
                                                           uint32_t rows_img, uint32_t d, uint32_t nch, unsigned char *img,
                                                           unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= rows_img) return;
  sketch_row(X, stride, w, w < n_src, d, nch, img, max_norm, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void sketch_rows_kernel(const float *__restrict__ X, size_t stride, const uint32_t *__restrict__ list,
                                                          uint32_t count, uint32_t rows_img, uint32_t d, uint32_t nch,
                                                          unsigned char *img, unsigned long long *max_norm) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= count) return;
  const uint32_t row = list[w];
  if (row >= rows_img) return;
  sketch_row(X, stride, row, true, d, nch, img, max_norm, threadIdx.x & 63);
}

// ---- the pass ---------------------------------------------------------------------------------
// A wave owns tiles t = wave, wave + waves, ...; each is nch + 1 one-KiB loads (lane l: row 64 t + l's 16 bytes), kU in
// flight in a register ring that runs on across tiles.  The query's two levels sit in LDS: chunk c's 16 bytes are
// wave-uniform, so a chunk costs one broadcast ds_read_b128 per level and eight v_dot4c_i32_i8.  The tile's last load is
// the rows' metadata: the lane then holds everything its row's interval needs, no other memory access.
template <int CAP>
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
  }
  __shared__ uint32_t s_counts[kWavesPerBlock];
  tk.merge_block(wib, kWavesPerBlock, s_counts, lane);
  if (wib == 0) tk.store(a.part_keys + (size_t)blockIdx.x * a.k, a.part_pay + (size_t)blockIdx.x * a.k, lane);
}

// ---- certification ------------------------------------------------------------------------------
constexpr int kCertThreads = 1024;
__global__ __launch_bounds__(kCertThreads) void sketch_certify_kernel(const uint64_t *__restrict__ keys, const Payload *__restrict__ pay,
                                                                      uint32_t lists, uint32_t kp, uint32_t k, uint32_t cap,
                                                                      uint32_t *__restrict__ rows, uint32_t *count, uint32_t *info) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_prefix, s_remaining, s_total, s_count, s_fail;
  const uint32_t m = lists * kp;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_prefix = 0;
    s_remaining = k;
    s_total = 0;
    s_count = 0;
    s_fail = 0;
  }
  // Kt: the k-th smallest key(lo) of the retained entries, 8 bits per pass
  uint32_t mask = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256; i += kCertThreads) hist[i] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    for (uint32_t i = tid; i < m; i += kCertThreads) {
      if (keys[i] == kEmptyKey) continue;
      const uint32_t v = orderable(pay[i].raw);
      if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0, b = 0;
      if (pass == 0)
        for (uint32_t j = 0; j < 256; ++j) s_total += hist[j];
      for (; b < 255; ++b) {
        if (cum + hist[b] >= s_remaining) break;
        cum += hist[b];
      }
      s_remaining -= cum;
      s_prefix = prefix | (b << shift);
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  const uint32_t kt = s_total <= k ? 0xffffffffu : s_prefix;  // (k or fewer entries in all: every one is a candidate)
  // collect, and check that no full list can have dropped a row with key(hi) <= Kt
  const int lane = tid & (kWave - 1), w = tid / kWave;
  for (uint32_t l = w; l < lists; l += kCertThreads / kWave) {
    bool full = true;
    uint32_t mx = 0;
    for (uint32_t j0 = 0; j0 < kp; j0 += kWave) {
      const uint32_t j = j0 + lane;
      bool empty = true;
      uint32_t lo = 0;
      if (j < kp) {
        const uint64_t key = keys[(size_t)l * kp + j];
        empty = key == kEmptyKey;
        lo = (uint32_t)(key >> 32);
        if (!empty) {
          mx = mx > lo ? mx : lo;
          if (lo <= kt) {
            const uint32_t pos = atomicAdd(&s_count, 1u);
            if (pos < cap) rows[pos] = pay[(size_t)l * kp + j].row;
          }
        }
      }
      if (__ballot(j < kp && empty)) full = false;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, kWave);
      mx = mx > other ? mx : other;
    }
    if (lane == 0 && full && mx <= kt) s_fail = 1;
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t cnt = s_count;
    const bool ok = !s_fail && cnt <= cap;
    *count = ok ? cnt : 0u;
    info[0] = ok ? 1u : 0u;
    info[1] = cnt;
    info[2] = kt;
    info[3] = 0u;
    __threadfence_system();
  }
}

}  // namespace

hipError_t launch_sketch_build(const float *X, size_t stride, uint32_t n_src, uint32_t rows_img, uint32_t d, void *img,
                               unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim || rows_img % kSketchTileRows) return hipErrorInvalidValue;
  if (rows_img == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch_build_kernel, dim3((rows_img + 3) / 4), dim3(256), 0, s, X, stride, n_src, rows_img, d,
                     sketch_ld8(d) / 16, static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
}

hipError_t launch_sketch_rows(const float *X, size_t stride, const uint32_t *list, uint32_t count, uint32_t rows_img, uint32_t d,
                              void *img, unsigned long long *max_norm, hipStream_t s) {
  if (d == 0 || d > kSketchMaxDim) return hipErrorInvalidValue;
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(sketch_rows_kernel, dim3((count + 3) / 4), dim3(256), 0, s, X, stride, list, count, rows_img, d,
                     sketch_ld8(d) / 16, static_cast<unsigned char *>(img), max_norm);
  return hipGetLastError();
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
  if (a.k <= (uint32_t)kSmallK) {
    hipError_t e = allow_lds(sketch_scan_kernel<kCapSmall>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sketch_scan_kernel<kCapSmall>, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  } else {
    hipError_t e = allow_lds(sketch_scan_kernel<kCapLarge>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sketch_scan_kernel<kCapLarge>, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_sketch_certify(const uint64_t *keys, const Payload *pay, uint32_t lists, uint32_t kp, uint32_t k, uint32_t cap,
                                 uint32_t *rows, uint32_t *count, uint32_t *info, hipStream_t s) {
  if (lists == 0 || kp == 0 || k == 0 || k > kp || !rows || !count || !info) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sketch_certify_kernel, dim3(1), dim3(kCertThreads), 0, s, keys, pay, lists, kp, k, cap, rows, count, info);
  return hipGetLastError();
}

}  // namespace vt

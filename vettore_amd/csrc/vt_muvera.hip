// vt_muvera.hip -- K10 / K10s: MUVERA fixed-dimensional encoding of multi-vector sets (gfx950), from a dense chunk of
// uploaded vectors (K10) or from the slab of a resident multi-vector store (K10s).
//
// Replaces encode (native/vettore/src/muvera.rs:26-74) under muvera_encode_query / _document, for a chunk of
// sets at once.  Layout and launch shape: MuveraArgs in vt_device.h.  The result is the reference's bit for bit:
//   * hash4 (muvera.rs:219-225) is 64-bit integer arithmetic; random_weight (:203-207) is the u64 -> f64
//     conversion (round to nearest even), an exact scaling by 2^-64, one rounding to f32, then `* 2 - 1` in f32
//     (two roundings: the build never contracts a*b+c);
//   * every dot product (:116-125, :149-158) is ONE lane's sequential f64 sum over the dimension index; each term is
//     the product of two f32 values, exact in f64 (48 significant bits, no underflow), so fused or not is the same;
//   * accumulate (:164-177) runs over the set's vectors in input order -- one wave walks them one after the
//     other --, rounds to f32 after every vector, and divides by the partition's running count in f64 (IEEE);
//   * the count sketch (:180-200) is, per output slot, the sequential f32-rounded sum over that slot's input
//     indices in increasing order: the order the reference's single loop visits them in.
// Each kernel sits beside its launcher.
#include "vt_scan.cuh"

namespace vt {
namespace dev {

namespace {

// muvera.rs:219-225
__host__ __device__ __forceinline__ uint64_t rotl64(uint64_t v, int s) { return (v << s) | (v >> (64 - s)); }
__host__ __device__ __forceinline__ uint64_t hash4(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  uint64_t x = a ^ rotl64(b, 17) ^ rotl64(c, 31) ^ rotl64(d, 47);
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// muvera.rs:203-207: (hash as f64 / u64::MAX as f64) as f32 * 2.0 - 1.0; u64::MAX as f64 == 2^64
__device__ __forceinline__ float random_weight(uint64_t seed, uint64_t r, uint64_t p, uint64_t j) {
  const double unit64 = (double)hash4(seed, r, p, j) * 0x1p-64;
  const float unit = (float)unit64;
  const float twice = unit * 2.0f;
  return twice - 1.0f;
}

// ---------------------------------------------------------------- the table: weights and signs, once per call
// table[(r * d + j) * C + c]: c < k the SimHash weight of (r, c, j); c >= k the sign of (r, c - k, j) under
// seed + 17 (muvera.rs:153) as +-1.0f.  Lanes that differ in c read adjacent words.
__global__ void muvera_table_kernel(uint64_t seed, uint32_t R, uint32_t d, uint32_t k, uint32_t C, float *table) {
  const size_t total = (size_t)R * d * C;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t c = (uint32_t)(i % C);
  const size_t rj = i / C;
  const uint32_t j = (uint32_t)(rj % d), r = (uint32_t)(rj / d);
  float w;
  if (c < k) w = random_weight(seed, r, c, j);
  else w = (hash4(seed + 17, r, c - k, j) & 1) == 0 ? 1.0f : -1.0f;
  table[i] = w;
}

// muvera.rs:164-177.  false: "encoding overflow" (the slot keeps its value).
__device__ __forceinline__ bool accumulate(float *slot, double value, int mode, uint32_t count) {
  const double current = (double)*slot;
  const double next = mode == 0 ? current + value : current + (value - current) / (double)count;
  // (a NaN or an infinity fails both comparisons: is_finite is implied)
  if (next >= -(double)FLT_MAX && next <= (double)FLT_MAX) {
    *slot = (float)next;
    return true;
  }
  return false;
}

// The SimHash partition of repetition group g from the wave's sign ballot: projection c of the group sits at bit
// g * C + c, and the reference shifts the earlier projections up (muvera.rs:126).
__device__ __forceinline__ uint32_t partition_of(uint64_t mask, uint32_t g, uint32_t C, uint32_t k) {
  if (k == 0) return 0;
  const uint64_t field = (mask >> (g * C)) & ((1ull << k) - 1);
  return (uint32_t)(__brevll(field) >> (64 - k));
}

// ---------------------------------------------------------------- the encode kernels
// One wave per (set, group of a.rg repetitions).  Lane l serves repetition r0 + l / C and table column l % C when
// the columns of a.rg repetitions fit in one wave; a repetition with more than 64 columns takes the wave alone and
// its lanes walk the columns in passes of 64 (the SimHash columns, fewer than 31, are all in the first pass).
// K10 (muvera_encode_kernel) and K10s (muvera_encode_slab_kernel) differ in where a set's vectors lie and in how one is
// loaded into LDS; what a wave is (encode_wave) and everything it does with a loaded vector (encode_vector) is shared.
struct EncodeWave {
  uint32_t lane, r0, rga;   // the first repetition this wave serves and how many
  uint32_t g, c1;           // this lane's repetition within the group and its column in the first pass
  bool live1, wide;
  float *out;               // the set's row of a.full
  uint32_t *cnt;            // [rga][P] partition counts (document mode; LDS or device memory), else null
};

// `lcnt`: the wave's counts in LDS, zeroed here when they are the ones in use (the barrier before the first vector's
// load stands between that and their first reader).
__device__ __forceinline__ EncodeWave encode_wave(const MuveraArgs &a, uint32_t *lcnt) {
  EncodeWave w;
  w.lane = threadIdx.x;
  const uint32_t set = (uint32_t)(blockIdx.x / a.groups);
  w.r0 = (uint32_t)(blockIdx.x % a.groups) * a.rg;
  w.rga = min(a.rg, a.R - w.r0);
  const uint32_t C = a.C, P = 1u << a.k;
  w.out = a.full + (size_t)set * a.out_size;
  w.cnt = nullptr;
  if (a.mode == 1) {
    if (a.counts) {
      w.cnt = a.counts + ((size_t)set * a.R + w.r0) * P;                  // (zeroed by the host; rg == 1)
    } else {
      w.cnt = lcnt;
      for (uint32_t i = w.lane; i < w.rga * P; i += kWave) w.cnt[i] = 0;
    }
  }
  w.wide = C > (uint32_t)kWave;
  w.g = w.wide || C == 0 ? 0u : w.lane / C;
  w.c1 = w.wide || C == 0 ? w.lane : w.lane - w.g * C;
  w.live1 = C != 0 && w.g < w.rga && w.c1 < C;
  return w;
}

// One vector, staged in xs[0 .. d) and visible to the whole wave: its dot products, the sign ballot, the partition
// counts and the slots it is accumulated into.  true: some slot answered "encoding overflow".
__device__ __forceinline__ bool encode_vector(const MuveraArgs &a, const EncodeWave &w, const float *xs) {
  const uint32_t lane = w.lane, r0 = w.r0, rga = w.rga, g = w.g, c1 = w.c1;
  const uint32_t d = a.d, C = a.C, k = a.k, pd = a.pd;
  const uint32_t P = 1u << k;
  const bool live1 = w.live1;
  float *out = w.out;
  uint32_t *cnt = w.cnt;
  bool failed = false;

  // first pass: every SimHash column and the first projection columns
  double dot = 0.0;
  if (live1) {
    const float *t = a.table + (size_t)(r0 + g) * d * C + c1;
    for (uint32_t j = 0; j < d; ++j) dot += (double)xs[j] * (double)t[(size_t)j * C];
  }
  const uint64_t mask = __ballot(live1 && c1 < k && dot >= 0.0);
  const uint32_t part = partition_of(mask, g, C, k);

  if (a.mode == 1) {  // counts[count_index] += 1 (muvera.rs:55): one lane per repetition of the group
    if (lane < rga) {
      uint32_t *slot = cnt + (size_t)lane * P + partition_of(mask, lane, C, k);
      *slot = *slot + 1;
    }
    __syncthreads();
  }

  if (a.identity) {
    // muvera.rs:141-146: the coordinates themselves, lanes over (repetition, coordinate)
    for (uint32_t i = lane; i < rga * d; i += kWave) {
      const uint32_t gi = i / d, q = i - gi * d;
      const uint32_t pi = partition_of(mask, gi, C, k);
      const uint32_t count = a.mode == 1 ? cnt[(size_t)gi * P + pi] : 1u;
      if (!accumulate(out + (size_t)(r0 + gi) * a.rep_size + (size_t)pi * pd + q, (double)xs[q], a.mode, count)) failed = true;
    }
  } else {
    const uint32_t count = a.mode == 1 && g < rga ? cnt[(size_t)g * P + part] : 1u;
    float *base = out + (size_t)(r0 + g) * a.rep_size + (size_t)part * pd;
    if (live1 && c1 >= k && !accumulate(base + (c1 - k), dot, a.mode, count)) failed = true;
    if (w.wide) {
      for (uint32_t c = lane + kWave; c < C; c += kWave) {
        const float *t = a.table + (size_t)r0 * d * C + c;
        double val = 0.0;
        for (uint32_t j = 0; j < d; ++j) val += (double)xs[j] * (double)t[(size_t)j * C];
        if (!accumulate(base + (c - k), val, a.mode, count)) failed = true;
      }
    }
  }
  return failed;
}

// K10: set s is rows [set_off[s], set_off[s + 1]) of a dense matrix, d floats apart.
__global__ __launch_bounds__(kWave) void muvera_encode_kernel(const MuveraArgs a) {
  extern __shared__ __align__(16) float lds[];
  float *xs = lds;                                                        // [d] the current vector
  const EncodeWave w = encode_wave(a, reinterpret_cast<uint32_t *>(lds + a.d));
  const uint32_t set = (uint32_t)(blockIdx.x / a.groups);
  const uint32_t v0 = a.set_off[set], v1 = a.set_off[set + 1];
  bool failed = false;
  for (uint32_t v = v0; v < v1; ++v) {
    const float *x = a.X + (size_t)v * a.d;
    __syncthreads();  // the last vector's readers are done (and the counts are zeroed)
    for (uint32_t j = w.lane; j < a.d; j += kWave) xs[j] = x[j];
    __syncthreads();
    if (encode_vector(a, w, xs)) failed = true;
  }
  if (failed) a.status[set] = kErrEncodingOverflow;
}

// K10s: set s is doc_cnt[s] rows from row doc_first[s] on of a store's slab, `stride` floats apart.  A row starts on 16
// bytes and its pad is zero, so it is staged whole, four floats a lane (xs holds `stride` floats; the pad is never read).
__global__ __launch_bounds__(kWave) void muvera_encode_slab_kernel(const MuveraSlabArgs s) {
  extern __shared__ __align__(16) float lds[];
  const MuveraArgs &a = s.a;
  float *xs = lds;                                                        // [stride] the current row
  const EncodeWave w = encode_wave(a, reinterpret_cast<uint32_t *>(lds + s.stride));
  const uint32_t set = (uint32_t)(blockIdx.x / a.groups);
  const uint32_t first = s.doc_first[set], n = s.doc_cnt[set];
  const uint32_t quads = s.stride / 4;
  bool failed = false;
  for (uint32_t v = 0; v < n; ++v) {
    const float4 *x = reinterpret_cast<const float4 *>(a.X + ((size_t)first + v) * s.stride);
    __syncthreads();  // the last vector's readers are done (and the counts are zeroed)
    for (uint32_t j = w.lane; j < quads; j += kWave) reinterpret_cast<float4 *>(xs)[j] = x[j];
    __syncthreads();
    if (encode_vector(a, w, xs)) failed = true;
  }
  if (failed) a.status[set] = kErrEncodingOverflow;
}

// ---------------------------------------------------------------- the count sketch
// muvera.rs:180-200 as a gather: one thread per (set, output slot) walks the slot's input indices in increasing
// order (list[off[s] .. off[s + 1]): index in the low 31 bits, bit 31 set = sign -1).
__global__ void muvera_sketch_kernel(const float *full, size_t out_size, uint32_t nsets, uint32_t final_dim,
                                     const uint32_t *off, const uint32_t *list, float *out, int *status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)nsets * final_dim) return;
  const uint32_t set = (uint32_t)(i / final_dim), s = (uint32_t)(i % final_dim);
  const float *in = full + (size_t)set * out_size;
  float acc = 0.0f;
  bool failed = false;
  for (uint32_t e = off[s]; e < off[s + 1]; ++e) {
    const uint32_t w = list[e];
    const float value = in[w & 0x7fffffffu];
    const float sign = (w >> 31) ? -1.0f : 1.0f;
    const double next = (double)acc + (double)(sign * value);
    if (next >= -(double)FLT_MAX && next <= (double)FLT_MAX) acc = (float)next;
    else failed = true;
  }
  out[i] = acc;
  if (failed) status[set] = kErrEncodingOverflow;
}

}  // namespace

}  // namespace dev

uint64_t muvera_hash4(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return dev::hash4(a, b, c, d); }

hipError_t launch_muvera_table(uint64_t seed, uint32_t R, uint32_t d, uint32_t k, uint32_t C, float *table, hipStream_t s) {
  const size_t total = (size_t)R * d * C;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(dev::muvera_table_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, seed, R, d, k, C, table);
  return hipGetLastError();
}

uint32_t muvera_reps_per_wave(uint32_t R, uint32_t k, uint32_t C, int mode) {
  uint32_t rg;
  if (C > (uint32_t)dev::kWave) rg = 1;
  else if (C == 0) rg = 16;  // (identity without SimHash: no dot product at all, lanes over coordinates only)
  else rg = (uint32_t)dev::kWave / C;
  // document mode: the group's partition counts share kMuveraLdsPartitions words of LDS (more partitions than
  // that: one repetition per wave, counts in device memory)
  if (mode == 1) rg = std::min<uint32_t>(rg, std::max<uint32_t>(1u, kMuveraLdsPartitions >> k));
  return std::max<uint32_t>(1u, std::min(rg, R));
}

size_t muvera_lds_bytes(const MuveraArgs &a) {
  size_t bytes = (size_t)a.d * sizeof(float);
  if (a.mode == 1 && !a.counts) bytes += ((size_t)a.rg << a.k) * sizeof(uint32_t);
  return std::max<size_t>(bytes, 16);
}

hipError_t launch_muvera_encode(const MuveraArgs &a, hipStream_t s) {
  if (a.nsets == 0) return hipSuccess;
  const size_t lds = muvera_lds_bytes(a);
  if (lds > dev::kMaxLds || a.rg == 0 || a.groups == 0 || (size_t)a.nsets * a.groups > 0x7fffffffull) return hipErrorInvalidValue;
  hipError_t e = dev::allow_lds(dev::muvera_encode_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::muvera_encode_kernel, dim3((uint32_t)((size_t)a.nsets * a.groups)), dim3(dev::kWave), lds, s, a);
  return hipGetLastError();
}

size_t muvera_slab_lds_bytes(const MuveraSlabArgs &s) {
  size_t bytes = (size_t)s.stride * sizeof(float);
  if (s.a.mode == 1 && !s.a.counts) bytes += ((size_t)s.a.rg << s.a.k) * sizeof(uint32_t);
  return std::max<size_t>(bytes, 16);
}

hipError_t launch_muvera_encode_slab(const MuveraSlabArgs &s, hipStream_t stream) {
  const MuveraArgs &a = s.a;
  if (a.nsets == 0) return hipSuccess;
  const size_t lds = muvera_slab_lds_bytes(s);
  if (lds > dev::kMaxLds || a.rg == 0 || a.groups == 0 || (size_t)a.nsets * a.groups > 0x7fffffffull) return hipErrorInvalidValue;
  if (s.stride < a.d || s.stride % 4 != 0 || !s.doc_first || !s.doc_cnt) return hipErrorInvalidValue;
  hipError_t e = dev::allow_lds(dev::muvera_encode_slab_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dev::muvera_encode_slab_kernel, dim3((uint32_t)((size_t)a.nsets * a.groups)), dim3(dev::kWave), lds, stream, s);
  return hipGetLastError();
}

hipError_t launch_muvera_sketch(const float *full, size_t out_size, uint32_t nsets, uint32_t final_dim, const uint32_t *off,
                                const uint32_t *list, float *out, int *status, hipStream_t s) {
  const size_t total = (size_t)nsets * final_dim;
  if (total == 0) return hipSuccess;
  if ((total + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dev::muvera_sketch_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, full, out_size, nsets,
                     final_dim, off, list, out, status);
  return hipGetLastError();
}

}  // namespace vt

// vt_ingest.hip -- what runs when rows arrive, move or leave (gfx950): K5 sign packing, the finite check, and the
// helpers that scatter ranks and pad, gather, land and swap-delete rows of the slab.  Each kernel is followed by
// its launcher.
#include "vt_common.cuh"

#include <algorithm>

namespace vt {

using namespace dev;

namespace {

// ---------------------------------------------------------------------------
// K5: sign packing (compress_sign_bits, distances.rs:413-423).  One wave per
// 64 coordinates: lane j tests v[j] >= 0.0, the wave ballot IS the word.
// tiled != 0 writes K4's [tile][pair][row][2] layout, else plain [row][word].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sign_pack_kernel(const float *__restrict__ rows, size_t stride, uint32_t n,
                                                        uint32_t d, uint64_t *__restrict__ bits, int tiled, int nonzero) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t W = (d + 63) / 64;
  const uint32_t pairs = (W + 1) / 2;
  const uint64_t total = (uint64_t)n * W;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / kWave);
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6); w < total; w += nwaves) {
    const uint32_t r = (uint32_t)(w / W), wi = (uint32_t)(w - (uint64_t)r * W);
    const uint32_t j = wi * 64 + lane;
    bool bit = false;
    if (j < d) {
      const float v = rows[(size_t)r * stride + j];
      bit = nonzero ? v != 0.0f : v >= 0.0f;
    }
    const uint64_t word = __ballot(bit);
    if (lane == 0) {
      const size_t at = tiled ? hamming_word_index(r, wi, pairs) : (size_t)w;
      bits[at] = word;
    }
  }
}

// K5 for the resident corpus (tiled layout, rows on the slab's 256-byte grid): a wave takes
// 256 consecutive floats of a row as one coalesced 1-KiB load (float4 per lane) -- four words of
// the row.  Component c of all 64 lanes is one ballot; word w of the four is the 16 ballot bits of
// lanes 16w..16w+15 of each component, interleaved (bit 4i + c), which lanes 0..3 do with shifts
// and masks.  One pass over the rows at streaming rate instead of a 256-byte load per wave.
__global__ __launch_bounds__(256) void sign_pack_tiled_kernel(const float *__restrict__ rows, size_t stride, uint32_t n,
                                                              uint32_t d, uint64_t *__restrict__ bits, int nonzero) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t W = (d + 63) / 64;
  const uint32_t pairs = (W + 1) / 2;
  const uint32_t segs = (d + 255) / 256;  // per row
  const uint64_t total = (uint64_t)n * segs;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / kWave);
  constexpr int U = 4;  // segments in flight per wave (one 1-KiB load each)
  for (uint64_t g0 = ((uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6)) * U; g0 < total; g0 += nwaves * U) {
    f32x4 v[U];
    uint32_t r[U], sg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t g = g0 + u;
      r[u] = (uint32_t)(g / segs);
      sg[u] = (uint32_t)(g - (uint64_t)r[u] * segs);
      const uint32_t j0 = sg[u] * 256 + (uint32_t)lane * 4;
      v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (g < total && j0 < stride) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(rows + (size_t)r[u] * stride + j0));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (g0 + u >= total) break;  // (wave-uniform)
      const uint32_t j0 = sg[u] * 256 + (uint32_t)lane * 4;
      const float c[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      uint64_t m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = __ballot(j0 + k < d && (nonzero ? c[k] != 0.0f : c[k] >= 0.0f));
      if (lane < 4) {
        const uint32_t wi = sg[u] * 4 + (uint32_t)lane;
        if (wi < W) {
          uint64_t word = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            uint64_t x = (m[k] >> (16 * lane)) & 0xffffull;  // bit i -> bit 4 i
            x = (x | (x << 24)) & 0x000000ff000000ffull;
            x = (x | (x << 12)) & 0x000f000f000f000full;
            x = (x | (x << 6)) & 0x0303030303030303ull;
            x = (x | (x << 3)) & 0x1111111111111111ull;
            word |= x << k;
          }
          bits[hamming_word_index(r[u], wi, pairs)] = word;
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_sign_pack(const float *rows, size_t stride, uint32_t n, uint32_t d, uint64_t *bits, int tiled,
                            hipStream_t s, int nonzero) {
  if (n == 0) return hipSuccess;
  if (tiled && stride % 4 == 0 && ((uintptr_t)rows & 15) == 0) {
    hipLaunchKernelGGL(sign_pack_tiled_kernel, dim3(4096), dim3(256), 0, s, rows, stride, n, d, bits, nonzero);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(sign_pack_kernel, dim3(2048), dim3(256), 0, s, rows, stride, n, d, bits, tiled, nonzero);
  return hipGetLastError();
}

namespace {

// K5 for a list of rows (bits of mutated rows patched in place, tiled layout).
__global__ __launch_bounds__(256) void sign_pack_rows_kernel(const float *__restrict__ rows, size_t stride,
                                                             const uint32_t *__restrict__ list, uint32_t count, uint32_t d,
                                                             uint64_t *__restrict__ bits, int nonzero) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t W = (d + 63) / 64;
  const uint32_t pairs = (W + 1) / 2;
  const uint64_t total = (uint64_t)count * W;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x / kWave);
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6); w < total; w += nwaves) {
    const uint32_t i = (uint32_t)(w / W), wi = (uint32_t)(w - (uint64_t)i * W);
    const uint32_t r = list[i];
    const uint32_t j = wi * 64 + lane;
    bool bit = false;
    if (j < d) {
      const float v = rows[(size_t)r * stride + j];
      bit = nonzero ? v != 0.0f : v >= 0.0f;
    }
    const uint64_t word = __ballot(bit);
    if (lane == 0) bits[hamming_word_index(r, wi, pairs)] = word;
  }
}

}  // namespace

hipError_t launch_sign_pack_rows(const float *rows, size_t stride, const uint32_t *list, uint32_t count, uint32_t d,
                                 uint64_t *bits, hipStream_t s, int nonzero) {
  if (count == 0) return hipSuccess;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(2048, ((uint64_t)count * ((d + 63) / 64) + 3) / 4);
  hipLaunchKernelGGL(sign_pack_rows_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, rows, stride, list, count, d, bits,
                     nonzero);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(256) void check_finite_kernel(const float *__restrict__ rows, size_t stride, uint32_t n,
                                                           uint32_t d, int *flag) {
  const uint64_t total = (uint64_t)n * d;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / d, c = i - r * d;
    bad |= !finite_f32(rows[r * stride + c]);
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

}  // namespace

hipError_t launch_check_finite(const float *rows, size_t stride, uint32_t n, uint32_t d, int *flag, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(check_finite_kernel, dim3(2048), dim3(256), 0, s, rows, stride, n, d, flag);
  return hipGetLastError();
}

namespace {

// dst[idx[i]] = val[i]: rank updates of a few rows without re-uploading the column.
__global__ __launch_bounds__(256) void scatter_u32_kernel(const uint32_t *__restrict__ pairs, uint32_t n,
                                                          uint32_t *__restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[pairs[2 * i]] = pairs[2 * i + 1];
}

}  // namespace

hipError_t launch_scatter_u32(const uint32_t *pairs, uint32_t n, uint32_t *dst, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_u32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pairs, n, dst);
  return hipGetLastError();
}

namespace {

__global__ __launch_bounds__(256) void pad_rows_kernel(const float *__restrict__ src, uint32_t n, uint32_t d,
                                                       float *__restrict__ dst, size_t dst_stride) {
  const uint64_t total = (uint64_t)n * dst_stride;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / dst_stride, c = i - r * dst_stride;
    dst[i] = c < d ? src[r * d + c] : 0.0f;
  }
}

}  // namespace

hipError_t launch_pad_rows(const float *src, uint32_t n, uint32_t d, float *dst, size_t dst_stride, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(pad_rows_kernel, dim3(2048), dim3(256), 0, s, src, n, d, dst, dst_stride);
  return hipGetLastError();
}

namespace {

// dst row map[2i + 1] <- src row map[2i] (first d columns; the rest of the dst row zeroed): rows
// of a device-resident batch that land scattered in the slab (upserts; a batch dealt to shards).
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, uint32_t d,
                                                          const uint32_t *__restrict__ map, uint32_t count,
                                                          float *__restrict__ dst, size_t dst_stride) {
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const float *from = src + (size_t)map[2 * i] * d;
    float *to = dst + (size_t)map[2 * i + 1] * dst_stride;
    for (uint32_t c = threadIdx.x; c < dst_stride; c += blockDim.x) to[c] = c < d ? from[c] : 0.0f;
  }
}

}  // namespace

hipError_t launch_gather_rows(const float *src, uint32_t d, const uint32_t *map, uint32_t count, float *dst,
                              size_t dst_stride, hipStream_t s) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(count < 4096 ? count : 4096), dim3(256), 0, s, src, d, map, count, dst,
                     dst_stride);
  return hipGetLastError();
}

namespace {

// A trickle of rows lands (host/vt_types.h, Shard::Landing): `stage` is a slot of PINNED HOST memory as the device sees it
// -- `count` rows of `ld` floats, already zero padded, then their slab rows (0xFFFFFFFF: an earlier occurrence of an id that
// comes again in the same batch -- skipped, the last one wins, flat.rs:270-281), then `nranks` id ranks for the rows
// rank_first .. of the rank column.  One launch instead of a copy per run of rows and another for the ranks: back to back
// on one stream a small copy costs as much device time as this whole kernel.  One block per row, 16-byte moves.
__global__ __launch_bounds__(256) void land_rows_kernel(const float *__restrict__ stage, uint32_t count, uint32_t ld,
                                                        float *__restrict__ X, uint32_t *__restrict__ rank_col,
                                                        uint32_t rank_first, uint32_t nranks) {
  const uint32_t *targets = reinterpret_cast<const uint32_t *>(stage + (size_t)count * ld);
  const uint32_t *ranks = targets + count;
  if (blockIdx.x == 0 && rank_col)
    for (uint32_t i = threadIdx.x; i < nranks; i += blockDim.x) rank_col[rank_first + i] = ranks[i];
  for (uint32_t j = blockIdx.x; j < count; j += gridDim.x) {
    const uint32_t t = targets[j];
    if (t == 0xFFFFFFFFu) continue;
    const float4 *from = reinterpret_cast<const float4 *>(stage + (size_t)j * ld);
    float4 *to = reinterpret_cast<float4 *>(X + (size_t)t * ld);
    for (uint32_t c = threadIdx.x; c < ld / 4; c += blockDim.x) to[c] = from[c];
  }
}

}  // namespace

hipError_t launch_land_rows(const float *stage_dev, uint32_t count, uint32_t ld, float *X, uint32_t *rank_col, uint32_t rank_first,
                            uint32_t nranks, hipStream_t s) {
  if (count == 0 || ld % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(land_rows_kernel, dim3(count), dim3(256), 0, s, stage_dev, count, ld, X, rank_col, rank_first, nranks);
  return hipGetLastError();
}

namespace {

// flat.rs:88-93 on the slab: the last row moves into the hole (with its rank, when the rank column is current) and its old
// place is zeroed -- rows n..cap are scanned by the last tile and must stay defined.  r == last: only the zeroing.  One
// launch where the host used to queue a copy, a rank copy and a memset.
__global__ __launch_bounds__(256) void swap_delete_kernel(float *__restrict__ X, uint32_t ld, uint32_t r, uint32_t last,
                                                          uint32_t *__restrict__ rank_col) {
  float4 *hole = reinterpret_cast<float4 *>(X + (size_t)r * ld);
  float4 *tail = reinterpret_cast<float4 *>(X + (size_t)last * ld);
  for (uint32_t c = threadIdx.x; c < ld / 4; c += blockDim.x) {
    if (r != last) hole[c] = tail[c];
    tail[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  if (threadIdx.x == 0 && rank_col && r != last) rank_col[r] = rank_col[last];
}

}  // namespace

hipError_t launch_swap_delete(float *X, uint32_t ld, uint32_t r, uint32_t last, uint32_t *rank_col, hipStream_t s) {
  if (ld % 4 != 0 || r > last) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swap_delete_kernel, dim3(1), dim3(256), 0, s, X, ld, r, last, rank_col);
  return hipGetLastError();
}

}  // namespace vt

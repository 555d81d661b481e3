// vt_scan.hip -- K1's dispatch (gfx950): the scan's shape, LDS budget and tile height, and which instantiation
// unit (vt_scan_*.hip) serves a launch; plus the bare-read yardstick the scan is measured against.
#include "vt_scan.cuh"

namespace vt {

using namespace dev;

namespace {

size_t scan_lds_for(const ScanShape &p, uint32_t k) {
  const size_t buf = k <= (uint32_t)kSmallK ? WaveTopK<kCapSmall>::lds_bytes() : WaveTopK<kCapLarge>::lds_bytes();
  return ((size_t)(p.q_global ? 0u : p.ld) + (size_t)kWavesPerBlock * p.tr * p.ss) * sizeof(float) + kWavesPerBlock * buf;
}

// A row too long for the query to share LDS with the panels: the query stays in global memory
// (ScanShape.q_global) and the run-time-op kernel serves the scan.  Returns the LDS bytes.
size_t scan_fit(ScanShape &p, uint32_t k) {
  size_t bytes = scan_lds_for(p, k);
  if (bytes > kMaxLds) {
    p.q_global = 1;
    bytes = scan_lds_for(p, k);
  }
  return bytes;
}

}  // namespace

size_t scan_lds_bytes(uint32_t d, uint32_t k) {
  ScanShape p;
  if (!make_scan_shape(d, 1, &p)) return 0;
  const size_t bytes = scan_fit(p, k);
  return bytes <= kMaxLds ? bytes : 0;
}

uint32_t scan_tile_rows(uint32_t n, uint32_t d, uint32_t resident_waves) {
  uint32_t want = kTileRows;
  if ((uint64_t)n <= (uint64_t)resident_waves * 8 * 8) want = 8;        // <= 8 tiles of 8 rows per wave
  else if ((uint64_t)n <= (uint64_t)resident_waves * 8 * 16) want = 16;
  ScanShape p;
  if (!make_scan_shape(d, n, &p, want)) return kTileRows;
  return p.tr;
}

hipError_t launch_scan(const ScanArgs &a, uint32_t blocks, hipStream_t s) {
  ScanDev sd;
  sd.a = a;
  if (!make_scan_shape(a.d, a.n, &sd.p, a.tile_rows ? a.tile_rows : (uint32_t)kTileRows)) return hipErrorInvalidValue;
  sd.p.tile_floats = sd.p.tr * (uint32_t)a.stride;
  const size_t lds = scan_fit(sd.p, a.k);
  if (lds > kMaxLds || a.k == 0 || a.k > (uint32_t)kMaxFusedK || a.stride < sd.p.ld || a.stride % 4 != 0)
    return hipErrorInvalidValue;
  if (a.gather != nullptr || sd.p.q_global) return launch_scan_general(sd, blocks, 1, lds, s);
  const bool padded = (a.d % kRowAlign) != 0;
  switch (metric_op(a.metric)) {
    case OP_DOT: return launch_scan_dot(sd, blocks, lds, padded, s);
    case OP_L2: return launch_scan_l2(sd, blocks, lds, padded, s);
    default: return launch_scan_misc(sd, blocks, lds, padded, s);
  }
}

hipError_t launch_scan_batch(const ScanArgs &a, uint32_t blocks, uint32_t nq, hipStream_t s) {
  ScanDev sd;
  sd.a = a;
  // candidate lists are short (tens to hundreds of rows per query): 8-row tiles spread a
  // list over more waves (a 32-row tile is ~25 us of one wave's load latency)
  if (!make_scan_shape(a.d, a.batch_cap, &sd.p, 8)) return hipErrorInvalidValue;
  sd.p.tile_floats = sd.p.tr * (uint32_t)a.stride;
  const size_t lds = scan_fit(sd.p, a.k);
  if (lds > kMaxLds || a.k == 0 || a.k > (uint32_t)kMaxFusedK || a.stride < sd.p.ld || !a.gather || !a.batch_counts)
    return hipErrorInvalidValue;
  return launch_scan_general(sd, blocks, nq, lds, s);
}

// The yardstick bench.py quotes beside the 8 TB/s spec figure (vt_device_read_peak): a read-only
// stream that does strictly less than any search kernel and reads the way the fastest of them do --
// the LDS-DMA ring of the batch passes (vt_batch_shadow.hip) with nobody consuming it.  A block of 8
// waves owns 384-KiB tiles of the buffer; wave w streams two 24-KiB runs of a tile KiB by KiB
// (global_load_lds_dwordx4 nt: 64 lanes x 16 B per piece) into its 2 KiB of each of five LDS stages,
// four chunks = 64 KiB per CU in flight behind a counted vmcnt.  Nothing is computed or written.
// (The piece is vt_nominate.cuh's dma16<true> written out: through the function this kernel's instructions come out in
// another order, and a yardstick's text does not change with a refactor of the things it measures.)
// (r03's yardstick -- 16-byte loads to registers strided over the whole grid, on a zero-filled buffer
// -- read SLOWER than the product's scan: a yardstick below the thing it measures is noise)
constexpr uint32_t kPeakStages = 5, kPeakRun = 24 * 1024, kPeakTile = 16 * kPeakRun;
__global__ __launch_bounds__(512, 1) void read_peak_kernel(const char *__restrict__ p, uint32_t ntiles) {
  extern __shared__ __align__(16) unsigned char peak_lds[];
  const uint32_t lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)peak_lds;
  const uint32_t off0 = (2 * wid) * kPeakRun + lane * 16, off1 = off0 + kPeakRun;
  uint32_t stage = 0;
  for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const char *base = p + (size_t)t * kPeakTile;
    for (uint32_t c = 0; c < kPeakRun / 1024; ++c) {
      stage = __builtin_amdgcn_readfirstlane(stage);
      const uint64_t b = reinterpret_cast<uint64_t>(base + (size_t)c * 1024);
      const uint64_t sb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
      const uint32_t m0a = lds0 + stage * 16384 + (2 * wid) * 1024, m0b = m0a + 1024;
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // this stage's previous two pieces (five chunks ago) have landed
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt" : : "s"(m0a), "v"(off0), "s"(sb) : "memory");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt" : : "s"(m0b), "v"(off1), "s"(sb) : "memory");
      stage = stage + 1 == kPeakStages ? 0u : stage + 1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(256) void peak_fill_kernel(uint32_t *p, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t h = (uint32_t)i * 2654435761u + 12345u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    p[i] = (h & 0x807fffffu) | 0x3f000000u;  // floats of either sign in [0.5, 1): random mantissas, like rows
  }
}

hipError_t launch_read_peak(const void *buf, size_t bytes, float *sink, uint32_t blocks, hipStream_t s) {
  (void)sink;
  const uint32_t ntiles = (uint32_t)(bytes / kPeakTile);  // (whole tiles only: read_peak_bytes() says how much that is)
  return launch_with_lds(read_peak_kernel, dim3(blocks), dim3(512), kPeakStages * 16384, s, reinterpret_cast<const char *>(buf), ntiles);
}
size_t read_peak_bytes(size_t bytes) { return bytes / kPeakTile * kPeakTile; }
hipError_t launch_peak_fill(void *buf, size_t bytes, hipStream_t s) {
  hipLaunchKernelGGL(peak_fill_kernel, dim3(4096), dim3(256), 0, s, reinterpret_cast<uint32_t *>(buf), bytes / 4);
  return hipGetLastError();
}

}  // namespace vt

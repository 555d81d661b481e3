// vt_sketch_batch.hip -- K1qm: a group of 2..8 dot-family or L2-family searches nominated from ONE pass over the int8 sketch
// of the rows (gfx950).  K1q (vt_sketch.hip) reads N (ld8 + 16) bytes per query; two to eight queries that travel
// together -- a small vt_flat_search_batch, or callers that met in the coalescer -- read them once here.
//
// The pass is K1q's: a wave owns tiles t = wave, wave + waves, ...; a ring of kU one-KiB non-temporal loads runs on across
// tiles; the tile's last load is the rows' metadata.  What changes is what meets a loaded chunk: every query's two int8
// levels (2 G integer sums per lane), read from LDS by broadcast ds_read_b128 as K1q reads its one query's -- a chunk's
// sixteen bytes of a level are wave-uniform.  At a finished tile each query g takes K1q's epilogue -- the same f64
// expression in the same order, with its own t1, t2, ||q||, ||eta||, kerr and ||q||^2 ends from the arguments' per-query
// arrays -- and offers to its own WaveTopK.  The integer dots are exact, so the two words (query g, row r) leaves are
// bit for bit what launch_sketch_scan gives for query g alone (tests/test_gpu_sketch_batch_kernels.py).
//
// G is compiled for 2, 4 and 8; a group in between runs the next one up with zero images in the unused places (their sums
// are formed and dropped: the epilogue and the lists are the ng queries' alone).  Lists: [ng][blocks][k'].
#include "vt_sketch.cuh"

#include "host/vt_sketchbatch.h"

namespace vt {

namespace {

static_assert(vt_host::kSketchBatchLdsLimit * 2 == kMaxLds, "two blocks of the group pass share a CU's LDS");
static_assert(vt_host::kSketchBatchWaveBuf == WaveTopK<kCapSmall>::lds_bytes(), "a wave's small buffer");
static_assert(vt_host::kSketchBatchWaves == kWavesPerBlock, "waves per block");
static_assert(vt_host::kSketchBatchMaxGroup == kSketchMultiMax, "the largest group on both sides");
static_assert(vt_host::kSketchBatchListMax == kSmallK, "lists that fit the small wave buffer");

template <int CAP, bool L2, int G>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void sketch_scan_multi_kernel(const SketchScanMultiArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t ld8 = a.nch * 16;
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32x4 *qlds = reinterpret_cast<const u32x4 *>(lds_raw);  // [G][2][nch]
  // query g's four wave buffers lie side by side (merge_block walks them)
  unsigned char *tkbase = lds_raw + (size_t)G * 2 * ld8;
  for (uint32_t i = threadIdx.x; i < (uint32_t)G * 2 * a.nch; i += blockDim.x)
    reinterpret_cast<u32x4 *>(lds_raw)[i] = reinterpret_cast<const u32x4 *>(a.qimg)[i];
  // (the queries' scalars: read where a tile ends, from LDS -- held in scalar registers across the loop, 7 G of them
  // crowd out the wave buffers' state and spill)
  __shared__ double s_par[G][8];
  if (threadIdx.x < (uint32_t)G) {
    const uint32_t g = threadIdx.x;
    s_par[g][0] = (double)a.t1[g];
    s_par[g][1] = (double)a.t2[g];
    s_par[g][2] = a.qn[g];
    s_par[g][3] = a.eta[g];
    s_par[g][4] = a.kerr[g];
    s_par[g][5] = a.qq_lo[g];
    s_par[g][6] = a.qq_hi[g];
    // K1's f32 products may be subnormal: an absolute 2^-126 per element covers them, flushed or not
    s_par[g][7] = ((double)a.d + 16.0) * 0x1p-125;
  }
  __syncthreads();

  WaveTopK<CAP> tk[G];
#pragma unroll
  for (int g = 0; g < G; ++g) tk[g].init(tkbase + (size_t)(g * kWavesPerBlock + wib) * WaveTopK<CAP>::lds_bytes(), a.k);
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

    uint32_t ct = wave, cc = 0;  // compute cursor
    int acc1[G], acc2[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc1[g] = acc2[g] = 0;
    while (ct < ntiles) {
      bool fin = false;
      int f1[G], f2[G];
#pragma unroll
      for (int g = 0; g < G; ++g) f1[g] = f2[g] = 0;
      u32x4 meta = u32x4{0u, 0u, 0u, 0u};
      uint32_t ftile = 0;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const u32x4 x = buf[u];
        buf[u] = load();
        if (ct < ntiles) {
          if (cc < a.nch) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const u32x4 q1 = qlds[(uint32_t)(2 * g) * a.nch + cc], q2 = qlds[(uint32_t)(2 * g + 1) * a.nch + cc];
              acc1[g] = __builtin_amdgcn_sdot4((int)x.x, (int)q1.x, acc1[g], false);
              acc1[g] = __builtin_amdgcn_sdot4((int)x.y, (int)q1.y, acc1[g], false);
              acc1[g] = __builtin_amdgcn_sdot4((int)x.z, (int)q1.z, acc1[g], false);
              acc1[g] = __builtin_amdgcn_sdot4((int)x.w, (int)q1.w, acc1[g], false);
              acc2[g] = __builtin_amdgcn_sdot4((int)x.x, (int)q2.x, acc2[g], false);
              acc2[g] = __builtin_amdgcn_sdot4((int)x.y, (int)q2.y, acc2[g], false);
              acc2[g] = __builtin_amdgcn_sdot4((int)x.z, (int)q2.z, acc2[g], false);
              acc2[g] = __builtin_amdgcn_sdot4((int)x.w, (int)q2.w, acc2[g], false);
            }
            ++cc;
          } else {  // the tile's metadata: the rows are complete (at most one per group: seg > kU)
            fin = true;
#pragma unroll
            for (int g = 0; g < G; ++g) {
              f1[g] = acc1[g];
              f2[g] = acc2[g];
              acc1[g] = acc2[g] = 0;
            }
            meta = x;
            ftile = ct;
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
        const uint32_t rank = valid ? (a.id_rank ? a.id_rank[row] : row) : 0u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if ((uint32_t)g >= a.ng) continue;  // (wave-uniform: a place the group does not fill)
          // K1q's epilogue (sketch_scan_kernel), expression for expression: the words must be the lone pass's
          const double t1 = s_par[g][0], t2 = s_par[g][1];
          const double qn = s_par[g][2], eta = s_par[g][3], kerr = s_par[g][4], tiny = s_par[g][7];
          const double av = s * (t1 * (double)f1[g] + t2 * (double)f2[g]);
          const double e = (qn * rho + eta * nu + kerr * qn * (nu + rho) + 0x1p-40 * nu * (qn + eta)) * kSlack + tiny;
          float khi_rank, klo_rank;  // key(lo) >= key(hi): the rank functions fall as the dot rises
          if constexpr (L2) {
            const double xxu = (double)__uint_as_float(meta.w), xxl = xxu * (1.0 - 0x1p-22);
            const double kappa = tiny * 0x1p102;  // ((d + 16) 2^-23, exactly: tiny is (d + 16) 2^-125, the scaling a power of two)
            const double qq_lo = s_par[g][5], qq_hi = s_par[g][6];
            const double delta = 0x1p-40 * (qq_hi + xxu + 2.0 * e);
            const double v_lo = fmax(0.0, qq_lo + xxl - 2.0 * (av + e) - delta);
            const double v_hi = qq_hi + xxu - 2.0 * (av - e) + delta;
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
          const uint64_t key = ((uint64_t)orderable(klo_rank) << 32) | rank;
          tk[g].offer(valid, key, row, khi_rank, lane);
        }
      }
    }
  }
  __shared__ uint32_t s_counts[G][kWavesPerBlock];
  static_assert(sizeof(s_par) + sizeof(s_counts) <= vt_host::kSketchBatchLdsStatic, "the static words the host leaves room for");
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if ((uint32_t)g >= a.ng) continue;  // (block-uniform: every wave skips the same places)
    tk[g].merge_block(wib, kWavesPerBlock, s_counts[g], lane);
    const size_t list = ((size_t)g * gridDim.x + blockIdx.x) * a.k;
    if (wib == 0) tk[g].store(a.part_keys + list, a.part_pay + list, lane);
  }
}

}  // namespace

uint32_t sketch_scan_multi_group(uint32_t ng) { return vt_host::sketch_batch_compiled_group(ng); }

size_t sketch_scan_multi_lds_bytes(uint32_t d, uint32_t k, uint32_t group) {
  if (d == 0 || d > kSketchMaxDim) return 0;
  return vt_host::sketch_batch_lds_bytes(d, k, group);
}

hipError_t launch_sketch_scan_multi(const SketchScanMultiArgs &a, uint32_t blocks, hipStream_t s) {
  if (a.ng < 2 || a.ng > (uint32_t)kSketchMultiMax) return hipErrorInvalidValue;
  const uint32_t group = sketch_scan_multi_group(a.ng);
  const size_t lds = sketch_scan_multi_lds_bytes(a.d, a.k, group);
  if (!lds || a.nch != sketch_ld8(a.d) / 16 || blocks == 0 || !a.img || !a.qimg || !a.part_keys || !a.part_pay) return hipErrorInvalidValue;
  const bool l2 = a.metric == M_L2 || a.metric == M_L2SQ;
  if (!l2 && a.metric != M_COS && a.metric != M_IP && a.metric != M_NIP) return hipErrorInvalidValue;
  auto launch = [&](auto kernel) -> hipError_t {
    hipError_t e = allow_lds(kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
    return hipGetLastError();
  };
  switch (group) {
    case 2: return l2 ? launch(sketch_scan_multi_kernel<kCapSmall, true, 2>) : launch(sketch_scan_multi_kernel<kCapSmall, false, 2>);
    case 4: return l2 ? launch(sketch_scan_multi_kernel<kCapSmall, true, 4>) : launch(sketch_scan_multi_kernel<kCapSmall, false, 4>);
    case 8: return l2 ? launch(sketch_scan_multi_kernel<kCapSmall, true, 8>) : launch(sketch_scan_multi_kernel<kCapSmall, false, 8>);
  }
  return hipErrorInvalidValue;
}

}  // namespace vt

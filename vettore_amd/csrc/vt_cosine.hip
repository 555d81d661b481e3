// vt_cosine.hip -- the exact f64 cosine of vector_top_k (gfx950): K6 rerank of a candidate list, K6b scan of a
// prefix of every row with fused top-k, K6b for eight queries a sweep; and K7 normalisation.  Each kernel is
// followed by its LDS formula and its launcher.
#include "vt_panel.cuh"

namespace vt {

using namespace dev;

namespace {

// K6 (cosine part): exact rerank value of distances.rs:160-177.  One wave per
// candidate: the wave stages the row and the query in LDS with coalesced loads,
// then lanes 0..2 run the three sequential f64 sums |q|^2, |x|^2, q.x in index
// order side by side (distances.rs:179-185 f64_dot is a sequential fold; products
// of two f32 are exact in f64, so only the order of the additions matters).
__global__ __launch_bounds__(64) void cosine_rerank_kernel(const CosineRerankArgs a0) {
  extern __shared__ __align__(16) float crs[];  // [ld] query, [ld] row
  CosineRerankArgs a = a0;
  if (gridDim.y > 1) {  // query y of a batch (launch_cosine_rerank_batch)
    const uint32_t y = blockIdx.y;
    a.q += (size_t)y * a.q_stride;
    if (a.gather) a.gather += (size_t)y * a.gather_qstride;
    a.out_keys += (size_t)y * a.n;
    a.out_pay += (size_t)y * a.n;
  }
  const uint32_t i = blockIdx.x;
  const int lane = threadIdx.x;
  if (a.n_dev && i >= *a.n_dev) {  // (a list shorter than its buffer: nothing behind its end)
    if (lane == 0) a.out_keys[i] = kEmptyKey;
    return;
  }
  const uint32_t src = a.gather ? a.gather[(size_t)i * a.gather_stride] : i;
  const uint32_t ld4 = (a.d + 3) / 4 * 4;
  float *qs = crs, *xs = crs + ld4;
  const float *x = a.X + (size_t)src * a.stride;
  if ((a.stride & 3u) == 0 && a.stride >= ld4) {  // (the query buffer is always padded to padded_dim)
    // every 16-B load of the row and of the query goes out before the first LDS store
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x);
    const f32x4 *q4 = reinterpret_cast<const f32x4 *>(a.q);
    const uint32_t n4 = ld4 / 4;
    for (uint32_t base = 0; base < n4; base += 4 * kWave) {
      f32x4 xv[4], qv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t j = base + u * kWave + lane;
        xv[u] = j < n4 ? x4[j] : f32x4{0, 0, 0, 0};
        qv[u] = j < n4 ? q4[j] : f32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t j = base + u * kWave + lane;
        if (j < n4) {
          *reinterpret_cast<f32x4 *>(xs + 4 * j) = xv[u];
          *reinterpret_cast<f32x4 *>(qs + 4 * j) = qv[u];
        }
      }
    }
  } else {
    for (uint32_t j = lane; j < a.d; j += kWave) {
      qs[j] = a.q[j];
      xs[j] = x[j];
    }
  }
  wave_lds_fence();
  double acc = 0.0;
  if (lane < 3) {
    const float *A = lane == 1 ? xs : qs;  // lane 0: q.q   lane 1: x.x   lane 2: q.x
    const float *B = lane == 0 ? qs : xs;
    // fma(x, y, acc) == acc + x*y here (the product of two f32 is exact in f64).  The chain is
    // one dependent f64 FMA per element; what it must never wait for is LDS: blocks of 16
    // elements, the NEXT block's eight ds_read_b128 issued before the current block's 16 FMAs
    // (one basic block: a plain `#pragma unroll` left an exit test between the steps and a
    // `s_waitcnt lgkmcnt(0)` in front of every four FMAs -- 30 cycles per element instead of 10).
    uint32_t j = 0;
    const uint32_t nblk = a.d / 16;
    if (nblk) {
      f32x4 a0[4], b0[4], a1[4], b1[4];  // two blocks in registers, filled and consumed in turn
      auto fetch = [&](f32x4(&ra)[4], f32x4(&rb)[4], uint32_t blk) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ra[u] = *reinterpret_cast<const f32x4 *>(A + 16 * blk + 4 * u);
          rb[u] = *reinterpret_cast<const f32x4 *>(B + 16 * blk + 4 * u);
        }
        __builtin_amdgcn_sched_barrier(0);  // the reads stay in front of the chain that hides them
      };
      // (the chain's first step is split off: the compiler waits for EVERY outstanding LDS read
      // before the first use of a block fetched an iteration ago, so the next fetch goes out
      // right after that step, not before it)
      auto head = [&](const f32x4(&ra)[4], const f32x4(&rb)[4]) {
        acc = __builtin_fma((double)ra[0].x, (double)rb[0].x, acc);
        __builtin_amdgcn_sched_barrier(0);
      };
      auto rest = [&](const f32x4(&ra)[4], const f32x4(&rb)[4]) {
        acc = __builtin_fma((double)ra[0].y, (double)rb[0].y, acc);
        acc = __builtin_fma((double)ra[0].z, (double)rb[0].z, acc);
        acc = __builtin_fma((double)ra[0].w, (double)rb[0].w, acc);
#pragma unroll
        for (int u = 1; u < 4; ++u) {
          acc = __builtin_fma((double)ra[u].x, (double)rb[u].x, acc);
          acc = __builtin_fma((double)ra[u].y, (double)rb[u].y, acc);
          acc = __builtin_fma((double)ra[u].z, (double)rb[u].z, acc);
          acc = __builtin_fma((double)ra[u].w, (double)rb[u].w, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      fetch(a0, b0, 0);
      uint32_t blk = 0;
      for (; blk + 2 <= nblk; blk += 2) {
        head(a0, b0);
        fetch(a1, b1, blk + 1);
        rest(a0, b0);
        head(a1, b1);
        fetch(a0, b0, blk + 2 < nblk ? blk + 2 : nblk - 1);  // (no next block: the last one again, unused)
        rest(a1, b1);
      }
      if (blk < nblk) {
        head(a0, b0);
        rest(a0, b0);
      }
      j = nblk * 16;
    }
    for (; j < a.d; ++j) acc = __builtin_fma((double)A[j], (double)B[j], acc);
  }
  const double qq = __shfl(acc, 0, kWave), xx = __shfl(acc, 1, kWave), qx = __shfl(acc, 2, kWave);
  if (lane != 0) return;
  float raw = cosine_raw(qx, sqrt(qq), sqrt(xx));  // distances.rs:160-177
  const bool ok = raw == raw;
  if (!ok) {
    atomicMax(a.status, kErrOverflow);
    raw = 0.0f;
  }
  const uint32_t rk = a.id_rank ? a.id_rank[src] : src;
  a.out_keys[i] = ok ? (((uint64_t)orderable(1.0f - raw) << 32) | rk) : kEmptyKey;
  Payload p;
  p.row = src;
  p.raw = raw;
  a.out_pay[i] = p;
}

}  // namespace

hipError_t launch_cosine_rerank(const CosineRerankArgs &a, hipStream_t s) { return launch_cosine_rerank_batch(a, 1, s); }

hipError_t launch_cosine_rerank_batch(const CosineRerankArgs &a, uint32_t nq, hipStream_t s) {
  if (a.n == 0 || nq == 0) return hipSuccess;
  const size_t lds = (size_t)2 * ((a.d + 3) / 4 * 4) * sizeof(float);
  if (lds > kMaxLds) return hipErrorInvalidValue;
  hipError_t e = allow_lds(cosine_rerank_kernel, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cosine_rerank_kernel, dim3(a.n, nq), dim3(64), lds, s, a);
  return hipGetLastError();
}

namespace {

// K6b: exact f64 cosine of a prefix of every row + fused top-k.  The reference
// folds |x|^2 and q.x sequentially in f64, element by element, so the K1 trick
// applies one level down: a wave owns 64 rows and walks them in panels of 32
// floats (PanelWalk, vt_panel.cuh), and lane r runs row r's two f64 chains over
// the parked panel -- 64 chains in parallel.
template <int CAP, int PANEL>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void cosine_scan_kernel(const CosineScanArgs a) {
  extern __shared__ __align__(16) float cs_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ldq = padded_dim(a.d);
  float *qs = cs_lds;
  unsigned char *tkbuf = reinterpret_cast<unsigned char *>(cs_lds + ldq + panel_lds_floats()) + wib * WaveTopK<CAP>::lds_bytes();
  for (uint32_t i = threadIdx.x; i < ldq; i += blockDim.x) qs[i] = a.q[i];
  __syncthreads();

  const double ln = sqrt(a.qq);

  WaveTopK<CAP> tk;
  tk.init(tkbuf, a.k);
  uint32_t my_rank;
  double xx, qx;
  walk_panels<PANEL>(
      a, 1u, cs_lds + ldq, lane, wib,
      [&](uint32_t, uint32_t grow) {
        my_rank = (grow < a.n && a.id_rank) ? a.id_rank[grow] : grow;
        xx = 0.0, qx = 0.0;
      },
      [&](uint32_t p, const float *Sr) {
        const uint32_t cnt = a.d - p * PANEL < (uint32_t)PANEL ? a.d - p * PANEL : (uint32_t)PANEL;
        const float *qp = qs + p * PANEL;
        // fma(x, y, acc) == acc + x*y here: the product of two f32 is exact in f64
        uint32_t j = 0;
        for (; j + 4 <= cnt; j += 4) {
          const f32x4 xv = *reinterpret_cast<const f32x4 *>(Sr + j);
          const f32x4 qv = *reinterpret_cast<const f32x4 *>(qp + j);
          xx = __builtin_fma((double)xv.x, (double)xv.x, xx);
          qx = __builtin_fma((double)qv.x, (double)xv.x, qx);
          xx = __builtin_fma((double)xv.y, (double)xv.y, xx);
          qx = __builtin_fma((double)qv.y, (double)xv.y, qx);
          xx = __builtin_fma((double)xv.z, (double)xv.z, xx);
          qx = __builtin_fma((double)qv.z, (double)xv.z, qx);
          xx = __builtin_fma((double)xv.w, (double)xv.w, xx);
          qx = __builtin_fma((double)qv.w, (double)xv.w, qx);
        }
        for (; j < cnt; ++j) {
          const double xd = (double)Sr[j];
          xx = __builtin_fma(xd, xd, xx);
          qx = __builtin_fma((double)qp[j], xd, qx);
        }
      },
      [&](uint32_t, uint32_t grow) {
        const bool valid_row = grow < a.n;
        float raw = cosine_raw(qx, ln, sqrt(xx));  // distances.rs:160-177
        bool valid = valid_row;
        if (raw != raw) {
          if (valid) atomicMax(a.status, kErrOverflow);
          valid = false;
          raw = 0.0f;
        }
        const uint64_t key = ((uint64_t)orderable(1.0f - raw) << 32) | my_rank;
        if (a.has_lo) valid = valid && key > a.lo_key;
        if (a.key_out) {
          if (valid_row) a.key_out[grow] = valid ? key : kEmptyKey;
        } else {
          tk.offer(valid, key, grow, raw, lane);
        }
      });
  if (a.key_out) return;
  __shared__ uint32_t s_counts[kWavesPerBlock];
  tk.merge_block(wib, kWavesPerBlock, s_counts, lane);
  if (wib == 0) tk.store(a.part_keys + (size_t)blockIdx.x * a.k, a.part_pay + (size_t)blockIdx.x * a.k, lane);
}

}  // namespace

size_t cosine_scan_lds_bytes(uint32_t d, uint32_t k) {
  const size_t buf = k <= (uint32_t)kSmallK ? WaveTopK<kCapSmall>::lds_bytes() : WaveTopK<kCapLarge>::lds_bytes();
  const size_t bytes = ((size_t)padded_dim(d) + panel_lds_floats()) * sizeof(float) + kWavesPerBlock * buf;
  return bytes <= kMaxLds ? bytes : 0;
}

hipError_t launch_cosine_scan(const CosineScanArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = cosine_scan_lds_bytes(a.d, a.k);
  if (lds == 0 || a.k == 0 || a.k > (uint32_t)kMaxFusedK || a.n == 0) return hipErrorInvalidValue;
  auto go = [&](auto kern) -> hipError_t {
    hipError_t e = allow_lds(kern, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
    return hipGetLastError();
  };
  if (a.k <= (uint32_t)kSmallK) return go(cosine_scan_kernel<kCapSmall, kPanelFloats>);
  return go(cosine_scan_kernel<kCapLarge, kPanelFloats>);
}

// K6b, several queries per sweep (GroupSweepArgs in vt_device.h).  The row walk is
// cosine_scan_kernel's (PanelWalk, vt_panel.cuh): lane r walks row r of the parked panel -- one x.x chain and nq q.x
// chains, each the single kernel's sequence of f64 FMAs.  The queries are wave-uniform: they come as f64 through
// the scalar cache (constant address space => s_load) and enter the FMAs as SGPR operands -- read
// from LDS as f32 like the single kernel's one query, eight queries cost 8 LDS reads and 32
// conversions per 4 row elements and lane beside the 36 FMAs, and the pass was LDS / VALU bound
// at 3.5 TB/s of prefix bytes.
template <int PANEL>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void cosine_scan_multi_kernel(const GroupSweepArgs a) {
  extern __shared__ __align__(16) float csm_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ldq = padded_dim(a.d);
  typedef const __attribute__((address_space(4))) double *cd_p;
  cd_p qd = (cd_p)(uintptr_t)a.Qd;
  const bool dense = a.sample != nullptr;
  const uint32_t step = dense ? a.sample_stride : 1u;  // dense: every step-th tile
  float tauv[kGroupSweepMax];
  group_thresholds(a, dense, tauv);
  double xx, qx[kGroupSweepMax];
  walk_panels<PANEL>(
      a, step, csm_lds, lane, wib,
      [&](uint32_t, uint32_t) {
        xx = 0.0;
#pragma unroll
        for (uint32_t q = 0; q < kGroupSweepMax; ++q) qx[q] = 0.0;
      },
      [&](uint32_t p, const float *Sr) {
        const uint32_t cnt = a.d - p * PANEL < (uint32_t)PANEL ? a.d - p * PANEL : (uint32_t)PANEL;
        cd_p qp = qd + p * PANEL;
        // fma(x, y, acc) == acc + x*y here: the product of two f32 is exact in f64
        uint32_t j = 0;
        for (; j + 4 <= cnt; j += 4) {
          const f32x4 xv = *reinterpret_cast<const f32x4 *>(Sr + j);
          const double x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z, x3 = (double)xv.w;
          xx = __builtin_fma(x0, x0, xx);
          xx = __builtin_fma(x1, x1, xx);
          xx = __builtin_fma(x2, x2, xx);
          xx = __builtin_fma(x3, x3, xx);
          // (all eight slots, unused ones zero: a branch between the queries puts a wait behind every
          // scalar load; straight-line, the eight loads go out together)
          double w[kGroupSweepMax][4];
#pragma unroll
          for (uint32_t q = 0; q < kGroupSweepMax; ++q) {
            cd_p wp = qp + q * ldq + j;
            w[q][0] = wp[0];
            w[q][1] = wp[1];
            w[q][2] = wp[2];
            w[q][3] = wp[3];
          }
#pragma unroll
          for (uint32_t q = 0; q < kGroupSweepMax; ++q) {
            qx[q] = __builtin_fma(w[q][0], x0, qx[q]);
            qx[q] = __builtin_fma(w[q][1], x1, qx[q]);
            qx[q] = __builtin_fma(w[q][2], x2, qx[q]);
            qx[q] = __builtin_fma(w[q][3], x3, qx[q]);
          }
        }
        for (; j < cnt; ++j) {
          const double xd = (double)Sr[j];
          xx = __builtin_fma(xd, xd, xx);
#pragma unroll
          for (uint32_t q = 0; q < kGroupSweepMax; ++q) qx[q] = __builtin_fma(qp[q * ldq + j], xd, qx[q]);
        }
      },
      [&](uint32_t ti, uint32_t grow) {
        // distances.rs:160-177, once per query
        const bool valid_row = grow < a.n;
        const double rn = sqrt(xx);
#pragma unroll
        for (uint32_t q = 0; q < kGroupSweepMax; ++q) {
          if (q >= a.nq) break;
          float raw = cosine_raw(qx[q], sqrt(a.qq[q]), rn);
          bool valid = valid_row;
          if (raw != raw) {
            if (valid && !dense) atomicMax(a.status, kErrOverflow);
            valid = false;
            raw = 0.0f;
          }
          group_file(a, dense, q, tauv[q], valid, raw, 1.0f - raw, raw, grow, ti, lane);
        }
      });
}

hipError_t launch_cosine_scan_multi(const GroupSweepArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = group_sweep_lds_bytes();
  if (!a.Qd || ((uintptr_t)a.Qd & 31) || a.nq == 0 || a.nq > kGroupSweepMax || a.n == 0 || a.d == 0) return hipErrorInvalidValue;
  if (a.sample ? (a.sample_stride == 0 || a.sample_rows == 0) : (!a.tau || !a.cand_keys || !a.cand_pay || !a.cand_count))
    return hipErrorInvalidValue;
  hipError_t e = allow_lds(cosine_scan_multi_kernel<kPanelFloats>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cosine_scan_multi_kernel<kPanelFloats>, dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

namespace {

// K7: normalize_l2 (distances.rs:350-361), one row per lane.
__global__ __launch_bounds__(64) void normalize_l2_kernel(const float *__restrict__ in, uint32_t n, uint32_t d,
                                                          float *__restrict__ out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float *x = in + (size_t)r * d;
  float *y = out + (size_t)r * d;
  double acc = 0.0;
  for (uint32_t j = 0; j < d; ++j) {
    const double v = (double)x[j];
    acc += v * v;
  }
  const double norm = sqrt(acc);
  if (norm == 0.0) {
    for (uint32_t j = 0; j < d; ++j) y[j] = 0.0f;
  } else {
    for (uint32_t j = 0; j < d; ++j) y[j] = (float)((double)x[j] / norm);
  }
}

}  // namespace

hipError_t launch_normalize_l2(const float *in, uint32_t n, uint32_t d, float *out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(normalize_l2_kernel, dim3((n + 63) / 64), dim3(64), 0, s, in, n, d, out);
  return hipGetLastError();
}

}  // namespace vt

// vt_prefix_multi.hip -- K1p: K1's arithmetic over the first d coordinates of every row for up to eight
// queries per sweep (gfx950).  GroupSweepArgs in vt_device.h says what it is for: stage 1 of funnel_search on an
// L2 / dot / L1 / Linf collection (collection.ex:245-260 -> search.rs:56-60 -> distances.rs:42-68) for several
// callers at once.
//
// A prefix is a narrow thing: 64..256 floats of a 768-float row, i.e. 256-B..1-KiB runs at the rows' 3-KiB stride.
// The walk is K6b's (PanelWalk, vt_panel.cuh): a wave parks a 64-row x 32-float panel in its own LDS slice -- eight
// 1-KiB loads (8 rows x 128 B each), the next panel's already on their way -- and then lane r walks row r, chunk by
// chunk.  What differs is the arithmetic, which is K1's to the bit: per 8-float chunk eight
// separately rounded elements (q*x, (q-x)^2, |q-x|; never an FMA), their horizontal combination in the lane order
// of wide::f32x8::reduce_add (`order`: the four orders of vt_scan.cuh's chunk_sum, here inside one lane), then
// acc = acc + chunk sum down the row and the scalar tail one element at a time.  The queries are wave-uniform:
// eight floats per query and chunk through the scalar cache, used as SGPR operands.
// Cost: 16 (dot) to 24 (L2) VALU instructions per query and chunk, 8 queries: 512..768 per 8-KiB panel and wave
// -- the kernel sits between the VALU and the prefix reads (DESIGN.md 5.3 has the measured rates).
#include "vt_panel.cuh"

namespace vt {

using namespace dev;

namespace {

template <int OP>
__device__ __forceinline__ float pm_elem(float q, float x) {
  return elem<OP>(0, q, x);
}

// wide::f32x8::reduce_add of one chunk's eight elements e[0..7], all in this lane (vt_scan.cuh chunk_sum: the even
// lane of a pair holds l0..l3, the odd one l4..l7)
template <int OP, int ORDER>
__device__ __forceinline__ float pm_reduce(const float (&e)[8]) {
  if (ORDER == 1)  // AVX: ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7))
    return comb<OP>(0, comb<OP>(0, comb<OP>(0, e[0], e[4]), comb<OP>(0, e[2], e[6])),
                    comb<OP>(0, comb<OP>(0, e[1], e[5]), comb<OP>(0, e[3], e[7])));
  if (ORDER == 2)  // SEQ: (((l0+l1)+l2)+l3) + (((l4+l5)+l6)+l7)
    return comb<OP>(0, comb<OP>(0, comb<OP>(0, comb<OP>(0, e[0], e[1]), e[2]), e[3]),
                    comb<OP>(0, comb<OP>(0, comb<OP>(0, e[4], e[5]), e[6]), e[7]));
  if (ORDER == 3)  // SSE2: ((l0+l2)+(l1+l3)) + ((l4+l6)+(l5+l7))
    return comb<OP>(0, comb<OP>(0, comb<OP>(0, e[0], e[2]), comb<OP>(0, e[1], e[3])),
                    comb<OP>(0, comb<OP>(0, e[4], e[6]), comb<OP>(0, e[5], e[7])));
  // PAIR: ((l0+l1)+(l2+l3)) + ((l4+l5)+(l6+l7))
  return comb<OP>(0, comb<OP>(0, comb<OP>(0, e[0], e[1]), comb<OP>(0, e[2], e[3])),
                  comb<OP>(0, comb<OP>(0, e[4], e[5]), comb<OP>(0, e[6], e[7])));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// One chunk of one query: acc' = acc (+|max) reduce_add(elements).  x / q as four pairs (l0,l1) (l2,l3) (l4,l5) (l6,l7) --
// the pairs a ds_read_b128 / s_load_dwordx8 deliver.  The SSE2 and AVX orders add pairs to pairs: the elements and the
// first levels of the tree are packed instructions over two ELEMENTS of one query (v_pk_mul_f32 / v_pk_add_f32; left to
// itself the compiler packs over two QUERIES instead and pays for it with a register move per operand pair).
template <int OP, int ORDER>
__device__ __forceinline__ float pm_chunk(float acc, const f32x2 (&x)[4], const f32x2 (&q)[4]) {
  if (OP == OP_L1 && (ORDER == 3 || ORDER == 1)) {
    // |q - x|: packed differences; the absolute values are operand modifiers of the (plain) adds that follow
    f32x2 t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = q[i] - x[i];
    auto ab = [](float v) { return __builtin_fabsf(v); };
    if (ORDER == 3)
      return acc + (((ab(t[0].x) + ab(t[1].x)) + (ab(t[0].y) + ab(t[1].y))) + ((ab(t[2].x) + ab(t[3].x)) + (ab(t[2].y) + ab(t[3].y))));
    return acc + (((ab(t[0].x) + ab(t[2].x)) + (ab(t[1].x) + ab(t[3].x))) + ((ab(t[0].y) + ab(t[2].y)) + (ab(t[1].y) + ab(t[3].y))));
  }
  if ((OP == OP_DOT || OP == OP_L2) && (ORDER == 3 || ORDER == 1)) {
    f32x2 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (OP == OP_DOT) {
        e[i] = q[i] * x[i];
      } else {
        const f32x2 t = q[i] - x[i];
        e[i] = t * t;
      }
    }
    if (ORDER == 3) {  // ((l0+l2)+(l1+l3)) + ((l4+l6)+(l5+l7))
      const f32x2 a = e[0] + e[1], b = e[2] + e[3];
      return acc + ((a.x + a.y) + (b.x + b.y));
    }
    // AVX: ((l0+l4)+(l2+l6)) + ((l1+l5)+(l3+l7))
    const f32x2 t = (e[0] + e[2]) + (e[1] + e[3]);
    return acc + (t.x + t.y);
  }
  float e[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[2 * i] = pm_elem<OP>(q[i].x, x[i].x);
    e[2 * i + 1] = pm_elem<OP>(q[i].y, x[i].y);
  }
  return comb<OP>(0, acc, pm_reduce<OP, ORDER>(e));
}

template <int OP, int ORDER, int PANEL>
__global__ __launch_bounds__(kWavesPerBlock *kWave) void prefix_multi_kernel(const GroupSweepArgs a) {
  extern __shared__ __align__(16) float pm_lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  typedef const __attribute__((address_space(4))) float *cf_p;
  cf_p qs = (cf_p)(uintptr_t)a.Q;
  const uint32_t qst = a.q_stride;
  const bool dense = a.sample != nullptr;
  const uint32_t step = dense ? a.sample_stride : 1u;  // dense: every step-th tile
  const uint32_t cfull = a.d / 8, tail = a.d % 8;
  float tauv[kGroupSweepMax];
  group_thresholds(a, dense, tauv);
  float acc[kGroupSweepMax];
  walk_panels<PANEL>(
      a, step, pm_lds, lane, wib,
      [&](uint32_t, uint32_t) {
#pragma unroll
        for (uint32_t q = 0; q < kGroupSweepMax; ++q) acc[q] = 0.0f;
      },
      [&](uint32_t p, const float *Sr) {
        const uint32_t c0 = p * (PANEL / 8);
        const uint32_t nfull = cfull > c0 ? (cfull - c0 < (uint32_t)(PANEL / 8) ? cfull - c0 : (uint32_t)(PANEL / 8)) : 0u;
        for (uint32_t c = 0; c < nfull; ++c) {
          const f32x4 xa = *reinterpret_cast<const f32x4 *>(Sr + c * 8);
          const f32x4 xb = *reinterpret_cast<const f32x4 *>(Sr + c * 8 + 4);
          const f32x2 x[4] = {f32x2{xa.x, xa.y}, f32x2{xa.z, xa.w}, f32x2{xb.x, xb.y}, f32x2{xb.z, xb.w}};
          cf_p qp = qs + (size_t)(c0 + c) * 8;
          // (all eight slots, straight-line, four queries' floats at a time: the scalar loads of a half go out together;
          // an unused slot reads a readable row)
#pragma unroll
          for (uint32_t h = 0; h < kGroupSweepMax; h += 4) {
            f32x2 w[4][4];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
#pragma unroll
              for (int l = 0; l < 4; ++l) w[q][l] = f32x2{qp[(size_t)(h + q) * qst + 2 * l], qp[(size_t)(h + q) * qst + 2 * l + 1]};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) acc[h + q] = pm_chunk<OP, ORDER>(acc[h + q], x, w[q]);
          }
        }
        // the scalar tail: the chunk after the last full one, element by element (distances.rs:212-216 and its siblings)
        if (tail && cfull >= c0 && cfull < c0 + (uint32_t)(PANEL / 8)) {
          const uint32_t cl = cfull - c0;
          cf_p qp = qs + (size_t)cfull * 8;
          for (uint32_t j = 0; j < tail; ++j) {
            const float xv = Sr[cl * 8 + j];
#pragma unroll
            for (uint32_t q = 0; q < kGroupSweepMax; ++q) acc[q] = comb<OP>(0, acc[q], pm_elem<OP>(qp[(size_t)q * qst + j], xv));
          }
        }
      },
      [&](uint32_t ti, uint32_t grow) {
        // distances.rs:42-68 compute(): value, finiteness, f64 recovery; :113-119 rank_value
        const bool valid_row = grow < a.n;
        const int metric = a.metric;
#pragma unroll
        for (uint32_t q = 0; q < kGroupSweepMax; ++q) {
          if (q >= a.nq) break;
          float raw = acc[q];
          if (metric == M_NIP) raw = -raw;
          else if (metric == M_L2) raw = finite_f32(raw) ? __builtin_sqrtf(raw) : raw;
          bool valid = valid_row;
          if (valid && !finite_f32(raw)) {
            raw = recover_overflow(metric, a.Q + (size_t)q * qst, a.X + (size_t)grow * a.stride, a.d);
            if (raw != raw) {
              if (!dense) atomicMax(a.status, kErrOverflow);
              valid = false;
            }
          }
          const float rank = metric == M_IP ? -raw : raw;
          // (-rank: larger = better, the order the sample's threshold is taken in)
          group_file(a, dense, q, tauv[q], valid, -rank, rank, raw, grow, ti, lane);
        }
      });
}

template <int OP, int ORDER>
hipError_t launch_pm(const GroupSweepArgs &a, uint32_t blocks, size_t lds, hipStream_t s) {
  hipError_t e = allow_lds(prefix_multi_kernel<OP, ORDER, kPanelFloats>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((prefix_multi_kernel<OP, ORDER, kPanelFloats>), dim3(blocks), dim3(kWavesPerBlock * kWave), lds, s, a);
  return hipGetLastError();
}

template <int OP>
hipError_t launch_pm_op(const GroupSweepArgs &a, uint32_t blocks, size_t lds, hipStream_t s) {
  switch (a.order) {
    case 1: return launch_pm<OP, 1>(a, blocks, lds, s);
    case 2: return launch_pm<OP, 2>(a, blocks, lds, s);
    case 3: return launch_pm<OP, 3>(a, blocks, lds, s);
    default: return launch_pm<OP, 0>(a, blocks, lds, s);
  }
}

}  // namespace

bool prefix_multi_supports(int metric) {
  return metric == M_L2 || metric == M_L2SQ || metric == M_IP || metric == M_NIP || metric == M_L1 || metric == M_LINF;
}

size_t group_sweep_lds_bytes() { return panel_lds_floats() * sizeof(float); }

hipError_t launch_prefix_multi(const GroupSweepArgs &a, uint32_t blocks, hipStream_t s) {
  if (!prefix_multi_supports(a.metric) || !a.Q || ((uintptr_t)a.Q & 31) || a.q_stride % 8 != 0 || a.q_stride < a.d || a.nq == 0 ||
      a.nq > kGroupSweepMax || a.n == 0 || a.d == 0 || a.stride < padded_dim(a.d) || a.order < 0 || a.order > 3)
    return hipErrorInvalidValue;
  if (a.sample ? (a.sample_stride == 0 || a.sample_rows == 0) : (!a.tau || !a.cand_keys || !a.cand_pay || !a.cand_count || !a.status))
    return hipErrorInvalidValue;
  const size_t lds = group_sweep_lds_bytes();
  switch (metric_op(a.metric)) {
    case OP_DOT: return launch_pm_op<OP_DOT>(a, blocks, lds, s);
    case OP_L2: return launch_pm_op<OP_L2>(a, blocks, lds, s);
    case OP_L1: return launch_pm_op<OP_L1>(a, blocks, lds, s);
    default: return launch_pm_op<OP_LINF>(a, blocks, lds, s);
  }
}

}  // namespace vt

// vt_panel.cuh -- the row-panel walk of K6b, K6bm (vt_cosine.hip) and K1p (vt_prefix_multi.hip), and the group epilogue of
// the latter two, stated here once.
//   * The walk: a wave owns tiles of 64 rows and reads a prefix of them panel by panel -- 64 rows x PANEL floats, read with
//     coalesced 16-B loads (kRowsPerLoad rows x PANEL floats per wave instruction), parked in the wave's own LDS slice
//     S[64][PANEL + 4] (stride 4 * odd), after which lane r walks row r.  The panel after the one being walked is already
//     on its way: its loads go out as soon as the current one has been parked, so a wave keeps a panel in flight through
//     its chain phase (without this K6b sat at 4.3 TB/s of prefix bytes; a plain strided read of the same bytes does 6.5).
//     The product runs PANEL = kPanelFloats = 32: 8 wave loads of 8 rows x 128 B, 9 KB of LDS per wave, half the prefetch
//     registers of the 64-float form it replaced, and 1-7 % ahead of it at the same two blocks per CU (DESIGN_APPENDIX A.15).
//   * The group epilogue (GroupSweepArgs in vt_device.h): the thresholds, once, through the scalar cache; one (query, row)
//     score filed as the dense sample's cell, the tile's maximum, or an entry of the query's list.
// The kernels give the walk their arithmetic as three functions: begin(ti, grow) at the head of a tile (grow: the row this
// lane walks), panel(p, Sr) per parked panel (Sr: the lane's row of it), finish(ti, grow) behind the tile's last panel.
// (One loop with the kernels' parts inlined into it, and a tile's eight row addresses taken once at its head, in so many
// words.  Left to find that itself the compiler folds the two prefetches into one behind a select of the addresses, whenever
// the walk's state sits in a struct or behind a function of its own: a tile's addresses are then computed again for every
// panel, or both tiles' addresses are held for the whole tile at 32 VGPRs more -- profiles/README.md, panel_walk/.)
#pragma once
#include "vt_scan.cuh"

namespace vt {
namespace dev {

namespace {

constexpr int kPanelRows = 64;    // rows per tile: one per lane
constexpr int kPanelFloats = 32;  // the product's PANEL

// floats of LDS a block's waves park their panels in
constexpr size_t panel_lds_floats() { return (size_t)kWavesPerBlock * kPanelRows * (kPanelFloats + 4); }

// `panels`: panel_lds_floats() of the block's LDS; step: the launch walks every step-th tile (dense mode; else 1)
template <int PANEL, class Args, class Begin, class Panel, class Finish>
__device__ __forceinline__ void walk_panels(const Args &a, uint32_t step, float *panels, int lane, int wib, const Begin &begin,
                                            const Panel &panel, const Finish &finish) {
  constexpr int kStride = PANEL + 4;  // floats between the panel's rows in LDS (4 * odd)
  constexpr int kLanesPerRow = PANEL / 4, kRowsPerLoad = kWave / kLanesPerRow, kLoads = kPanelRows / kRowsPerLoad;
  float *S = panels + wib * (kPanelRows * kStride);  // this wave's slice
  const uint32_t total_waves = gridDim.x * kWavesPerBlock;
  const uint32_t wave_global = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t ntiles_all = (a.n + kPanelRows - 1) / kPanelRows;
  const uint32_t ntiles = (ntiles_all + step - 1) / step;  // tiles this launch walks
  const uint32_t npanel = (a.d + PANEL - 1) / PANEL;
  f32x4 v[kLoads];                                                          // the panel on its way
  const int lrow = lane / kLanesPerRow, lcol = (lane % kLanesPerRow) * 4;  // this lane's row within a load, its column
  // where this lane reads from in the eight loads of a panel of the launch's tile ti; a row past the end reads the last row
  auto aim = [&](uint32_t ti, const float *(&rp)[kLoads]) {
    const uint32_t t = ti * step;
#pragma unroll
    for (int s = 0; s < kLoads; ++s) {
      uint32_t r = t * kPanelRows + kRowsPerLoad * s + lrow;
      r = r < a.n ? r : a.n - 1;
      rp[s] = a.X + (size_t)r * a.stride + lcol;
    }
  };
  // panel p of the tile aimed at into the registers
  auto issue = [&](const float *const (&rp)[kLoads], uint32_t p) {
#pragma unroll
    for (int s = 0; s < kLoads; ++s) v[s] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(rp[s] + p * PANEL));
  };
  if (wave_global < ntiles) {
    const float *rp[kLoads];
    aim(wave_global, rp);
    issue(rp, 0);
  }
  for (uint32_t ti = wave_global; ti < ntiles; ti += total_waves) {
    const uint32_t grow = ti * step * kPanelRows + lane;
    begin(ti, grow);
    const float *rowp[kLoads];
    aim(ti, rowp);
    for (uint32_t p = 0; p < npanel; ++p) {
#pragma unroll
      for (int s = 0; s < kLoads; ++s) *reinterpret_cast<f32x4 *>(S + (kRowsPerLoad * s + lrow) * kStride + lcol) = v[s];
      wave_lds_fence();
      // the panel is parked; the next one goes out: the tile's next, else panel 0 of the wave's next tile
      if (p + 1 < npanel) {
        issue(rowp, p + 1);
      } else if (ti + total_waves < ntiles) {
        const float *rp[kLoads];
        aim(ti + total_waves, rp);
        issue(rp, 0);
      }
      panel(p, S + lane * kStride);
      wave_lds_fence();  // (the lanes are through with the parked panel)
    }
    finish(ti, grow);
  }
}

// ---- the group epilogue of K6bm and K1p -------------------------------------------------------------------------------
// The thresholds, once, through the scalar cache (+inf for the unused slots and in dense mode): read per tile as vector loads
// they each brought an s_waitcnt vmcnt(0) into the epilogue -- eight times per tile the wave waited for its NEXT tile's panel
// loads.
__device__ __forceinline__ void group_thresholds(const GroupSweepArgs &a, bool dense, float (&tauv)[kGroupSweepMax]) {
  typedef const __attribute__((address_space(4))) float *cf_p;
#pragma unroll
  for (uint32_t q = 0; q < kGroupSweepMax; ++q) tauv[q] = INFINITY;
  if (!dense) {
    cf_p tp = (cf_p)(uintptr_t)a.tau;
#pragma unroll
    for (uint32_t q = 0; q < kGroupSweepMax; ++q)
      if (q < a.nq) tauv[q] = tp[q];
  }
}

// Files the score of (query q, row grow of tile ti).  `good`: the score, larger = better -- the order the sample's
// threshold is taken in; `rank`: the value the key is built from; `valid`: the row exists and the pair has a score.
//   dense: good (-inf when !valid) to the sample's cell, or the tile's maximum to its one cell (sample_maxima);
//   sweep: good >= tau appends (key, {row, raw}) to the query's list -- cand_count[q] counts every such pair, those
//     past cand_cap are not stored.
__device__ __forceinline__ void group_file(const GroupSweepArgs &a, bool dense, uint32_t q, float tau, bool valid, float good, float rank, float raw,
                                           uint32_t grow, uint32_t ti, int lane) {
  if (dense) {
    if (a.sample_maxima) {  // the tile's best score, one value per query and tile
      float m = valid ? good : -INFINITY;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kWave));
      if (lane == 0 && ti < a.sample_rows) a.sample[(size_t)q * a.sample_rows + ti] = m;
      return;
    }
    const uint32_t i = ti * kPanelRows + lane;  // position in the sample
    if (i < a.sample_rows) a.sample[(size_t)q * a.sample_rows + i] = valid ? good : -INFINITY;
    return;
  }
  const bool hit = valid && good >= tau;
  const uint64_t m = __ballot(hit);
  if (m) {
    uint32_t base = 0;
    if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(&a.cand_count[q], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(m), kWave);
    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (hit && pos < a.cand_cap) {
      // (the id rank only here, in the rare lanes that list a row: a load per tile would be one more wait on vmcnt)
      const uint32_t my_rank = a.id_rank ? a.id_rank[grow] : grow;
      a.cand_keys[(size_t)q * a.cand_cap + pos] = ((uint64_t)orderable(rank) << 32) | my_rank;
      Payload pv;
      pv.row = grow;
      pv.raw = raw;
      a.cand_pay[(size_t)q * a.cand_cap + pos] = pv;
    }
  }
}

}  // namespace

}  // namespace dev
}  // namespace vt

// vt_sketchtiers.h -- the sketch tiers of a lone search (K1n, K1f, K1s, K1q) as one table, and the one gate
// that says which of them a search wants.  Stand-alone on purpose (no HIP, no header of the library): vt_types.h indexes the
// shard's columns by the tier, vt_sketchsearch.h fills the gate's shape from the shard and the settings and ties the
// constants to the device side's with static_asserts, and tests/sketch_gate_check.cpp builds it with plain g++ under
// AddressSanitizer and UBSan.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vt_host {

// The tiers, narrowest first: the order a lone search tries them in -- each the fallback of the one before it, and each
// wanted only where the next is -- and the order the slab takes their room back in.
enum SketchTierId : int { kTier4 = 0, kTier5, kTier6, kTier8, kSketchTierCount };
constexpr int kNibbleTierCount = kTier8;  // (the tiers before the int8 one: one pass skeleton, one chain, nibble_search)

constexpr uint32_t kSketchGateMaxDim = 32768;  // vt_device.h kSketchMaxDim
constexpr uint32_t kSketchListMax = 256;       // vt_device.h kMaxFusedK: a block's list fits one wave buffer
// K1q's lists: k' = max(2k, k + 16)
constexpr uint32_t sketch_list_k(size_t limit) { return (uint32_t)std::max<size_t>(2 * limit, limit + 16); }

struct SketchTierRow {
  int bits;                     // per element
  double min_bytes;             // f32 rows below this are served by the next tier (the dot family)
  double min_bytes_l2;          // the L2 family's own cut; 0: the tier's pass has no L2 epilogue, it never serves the family
  size_t max_limit;
  uint32_t list_k;              // entries of a block's list; 0: sketch_list_k(limit)
  uint32_t cand_cap;            // candidates the gathered K1 rescores at most (more: not certified)
  uint32_t rescore_blocks;      // the gathered K1's grid
  uint32_t miss_limit;          // passes in a row that did not certify before the shard stops taking the tier (0: none counted)
  uint32_t block_lists;         // lists a block of the pass leaves
  bool exact_threshold;         // Kt' from launch_sketch_refine
  bool best_rows;               // where the corpus gives every wave of the pass a tile: Kt'' from each list's best rows, inside the pass
  long off_at;                  // the value of its setting (`sketch` for the int8 tier, `sketch6` for the others) that switches it off
  long forced_from;             // force_sketch6 from this value on lifts min_bytes (1: any non-zero value; the int8 tier: or force_sketch)
};

// K1n (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1f applies, limits up to its max_limit over f32 rows
// of at least its min_bytes read the 4-bit sketch first -- 0.806 of the 5-bit sketch's bytes.  Its intervals are twice
// K1f's again: under the sketch's own threshold Kt a quarter of the corpus would be a candidate.  The threshold is therefore
// taken from the exact keys of the k rows with the smallest key(lo) (launch_sketch_refine, between the threshold and the
// collect kernels): the band is then one interval wide, not two, and leaves what K1f leaves behind Kt (tens of thousands
// of 10 M uniform unit rows at d = 768), over a wider spread -- so the pass leaves two lists a block, the candidate list
// has a row for every slot of those and the gathered K1 runs on its rescore_blocks blocks.  Where the corpus gives every wave
// of the pass a tile (best_rows; vt_sketchsearch.h, nibble_best_rows) the exact keys come from each list's two best rows,
// rescored by the wave that stores the list, and the threshold is their k-th smallest, found in the rescoring kernel's
// head: no threshold and no refine launch.  K1f is its fallback, on
// K1f's own terms; after miss_limit passes in a row that did not certify the shard stops taking K1n until the
// column is built anew.  The settings are K1s's, one value further still (the product's list of settings stays as long
// as it was): VT_SKETCH6=3 keeps K1s and K1f and switches K1n off -- the chain as it was without this column --;
// force_sketch6 = 1 / 2 select what they did, force_sketch6 = 3 forces all three.
// min_bytes: the sweep over sizes has not been run for any of the three cuts; this one stays at the one size the
// path has been measured at, which is K1s's and K1f's.
// cand_cap: every retained slot, 2 048 lists of 64.
//
// K1f (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1s applies, limits up to its max_limit over f32 rows
// of at least its min_bytes read the 5-bit sketch first -- 0.838 of the 6-bit sketch's bytes.  Its intervals are twice as
// wide and leave thousands of candidates (about 19 000 of 10 M uniform unit rows at d = 768), so its candidate list has a
// row for every retained slot of the block lists and the gathered K1 behind it runs on its rescore_blocks blocks (8-row
// tiles, a wave each: 2 048 waves keep 16 MB in flight over a list of some 58 MB).  K1s is its fallback, on K1s's own terms;
// after miss_limit passes in a row that did not certify the shard stops taking K1f until the column is built anew.
// The settings are K1s's, one value further (the product's list of settings stays as long as it was): VT_SKETCH6=2 keeps
// K1s and switches K1f off (0: both); force_sketch6 = 1 never selects K1f, force_sketch6 = 2 forces both.
// max_limit: on the headline corpus 300 queries at limit 10 left 12 147 ... 38 087 candidates (mean 22 758) and none
// missed; at limit 16 (mean 30 267, up to 40 685: the lists saturate) 7 missed, over the 1 % a miss's extra pass may cost
// (profiles/sketch5/candidates.json).
// min_bytes: the sweep over sizes has not been run; the cut stays at the one size the path has been measured at
// (DESIGN 5), which is K1s's.
// cand_cap: every retained slot, 1 024 lists of 64.
//
// K1s (vt_sketch_nibble.hip; its tail: vt_sketch.hip): where K1q applies, limits up to its max_limit over f32 rows of
// at least its min_bytes read the 6-bit sketch instead -- 0.755 of the int8 sketch's bytes -- with block lists of list_k
// entries; its wider intervals leave hundreds of candidates, which always go through the gathered K1.  The int8 pass is
// its fallback: a pass that does not certify is followed by K1q, and after miss_limit such passes in a row the
// shard stops taking K1s until the column is built anew (spiky rows never certify: DESIGN 4.10).  force_sketch alone
// never selects it.
// min_bytes: the chain behind the pass (certify-only tail 40 us, gathered K1 16, select 8.5 against K1q's tail of
// 26: +39 us in the headline's trace) is paid back at 26 ps per row (592 B at 6.63 TB/s against 784 B at 6.79 TB/s), i.e.
// near 1.5 M rows of d = 768 = 4.6 GB of f32 rows.  That is an estimate from two traces: the sweep over sizes that would
// place the meeting point has not been run, so the cut stays where the path has been measured to win.  Rows
// below it are served exactly as before.
// cand_cap: ~100 MB of f32 rows at d = 768.
//
// K1q (vt_sketch.hip): a lone cosine / inner-product / L2 search over rows of at least its min_bytes reads the
// int8 sketch -- a quarter of the bytes -- and the exact K1 rescores the rows it cannot rule out.  Only on strictly
// ranked shards (lazy searches after trickle inserts keep K1), and only while each block's list of k' = max(2k, k + 16)
// fits one wave buffer (max_limit).
// min_bytes: f32 rows below this take K1.  (With the pass's tail in one kernel the two paths meet near 130 MB of f32 rows,
// DESIGN 5; the cut stays where the suite's launch counters on mid-size corpora were written against it.)
// min_bytes_l2: the L2 family's own cut.  The family has been measured at 5 M and 10 M rows of d = 768 and in a sweep down
// to 256 MB; the cut does not sit at the measured meeting point but at 1 GiB, above the 461-MB shards whose lone
// L2 searches the two-rank rehearsal of config 4 prices as scans of the f32 rows.  L2 rows below it are served as before.
// The L2 family (L2, squared L2) reads the int8 sketch alone -- its column keeps ||x_r||^2 beside the dot's bounds (DESIGN
// 4.10); the 6-, 5- and 4-bit tiers stay with the dot family (their passes have no such epilogue).
// (force_sketch6 brings the int8 sketch with it: it is the 6-bit pass's fallback, and serves the limits that pass declines.)
constexpr double kSketchMiB = 1 << 20;
constexpr SketchTierRow kSketchTiers[kSketchTierCount] = {
    //   min_bytes            min_bytes_l2        limit  k'  cand_cap  blocks misses lists exact  best   off forced
    {4, 16.0 * 1024 * kSketchMiB, 0.0,                10, 64, 131072, 1024, 4, 2, true,  true,  3, 3},
    {5, 16.0 * 1024 * kSketchMiB, 0.0,                10, 64, 65536,  512,  4, 1, false, false, 2, 2},
    {6, 16.0 * 1024 * kSketchMiB, 0.0,                32, 64, 32768,  256,  4, 1, false, false, 0, 1},
    {8, 256.0 * kSketchMiB,       1024.0 * kSketchMiB, 128, 0, 4096,   32,   0, 1, false, false, 0, 1},
};
static_assert(!kSketchTiers[kTier5].best_rows && !kSketchTiers[kTier6].best_rows && !kSketchTiers[kTier8].best_rows &&
                  (!kSketchTiers[kTier4].best_rows || kSketchTiers[kTier4].exact_threshold),
              "only the 4-bit pass rescores its lists' best rows, and only in place of the refine");
static_assert(sketch_list_k(kSketchTiers[kTier8].max_limit) <= kSketchListMax &&
                  sketch_list_k(kSketchTiers[kTier8].max_limit + 1) > kSketchListMax,
              "the int8 tier's limits are those whose list fits one wave buffer");
// (the nibble tiers share the pass's list length)
constexpr uint32_t kSketchNibbleListK = kSketchTiers[kTier6].list_k;
static_assert(kSketchTiers[kTier4].list_k == kSketchNibbleListK && kSketchTiers[kTier5].list_k == kSketchNibbleListK, "one list length");

enum SketchFamily : int { kSketchNoFamily = 0, kSketchDot, kSketchL2 };

// What the gate looks at, as plain values (vt_sketchsearch.h fills it from the shard and the settings).
struct SketchGateShape {
  SketchFamily family = kSketchNoFamily;  // the handle's metric family (neither: no sketch serves it)
  bool ranks_clean = false;               // the rank column is strictly current
  bool single_nominate = false;           // lone searches go through the shadow
  bool no_rows = false;                   // n == 0
  long dim = 0;
  double row_bytes = 0.0;                 // n * ld * 4: the f32 rows
  long sketch = 1, sketch6 = 1, force_sketch = 0, force_sketch6 = 0;  // the settings
  bool refused[kSketchTierCount] = {};    // the tier's column could not be had
  bool pass_fits[kSketchTierCount] = {};  // the tier's pass takes rows of `dim` with its list (its *_scan_lds_bytes is not 0)
};

// The tiers a lone search of `limit` hits wants, as a mask of 1 << SketchTierId.  Nested: a tier is wanted only where every
// wider one is.
inline unsigned sketch_tiers_wanted(const SketchGateShape &s, size_t limit) {
  if (s.family == kSketchNoFamily || s.single_nominate || !s.ranks_clean || s.no_rows) return 0;
  if (s.dim <= 0 || s.dim > (long)kSketchGateMaxDim || limit == 0) return 0;
  unsigned mask = 0;
  for (int t = kSketchTierCount; t-- > 0;) {
    const SketchTierRow &r = kSketchTiers[t];
    const bool int8 = t == kTier8;
    const double cut = s.family == kSketchL2 ? r.min_bytes_l2 : r.min_bytes;
    if (s.family == kSketchL2 && r.min_bytes_l2 == 0.0) break;
    if ((int8 ? s.sketch : s.sketch6) == r.off_at || s.refused[t] || !s.pass_fits[t] || limit > r.max_limit) break;
    const bool forced = (r.forced_from <= 1 ? s.force_sketch6 != 0 : s.force_sketch6 >= r.forced_from) || (int8 && s.force_sketch != 0);
    if (!forced && !(s.row_bytes >= cut)) break;
    mask |= 1u << t;
  }
  return mask;
}

}  // namespace vt_host

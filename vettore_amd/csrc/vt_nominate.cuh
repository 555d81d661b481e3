// vt_nominate.cuh -- what the matrix-core nomination passes share: K2 (vt_batch.hip), K2b (vt_batch_bf16.hip) and
// K2s (vt_batch_shadow.hip).
//
// Each pass is ONE sequence of 32-k chunks running through all of a block's row tiles, carried by a ring of LDS
// stages that LDS-DMA fills, and ends every tile in an epilogue that files scores.  Here, once: the DMA piece, the
// bf16 packing, the tile sequence and the DMA cursor that walks it, the accumulator layouts, the L2 rank term and its
// norm fetch, the filing of one candidate, and the host side of a launch.  What
// stays in each unit is what makes that kernel itself: operand shapes, ring depth and wait counts, where its DMA
// pieces and fragment reads sit among its MFMAs, its sched_* barriers -- the chunk loops differ on purpose, and each
// unit's comments record the measurements behind its shape.
#pragma once
#include "vt_common.cuh"

// Timing experiments on K2 and K2b (tools/batch_debug.sh, tools/k2b_probe.hip) remove barriers, waits and DMA from
// the hot loop: results are garbage with any bit set, and the host's acceptance test cannot tell.  They exist only in
// builds made with -DVT_BATCH_TIMING_EXPERIMENTS (make experiments); the product library ignores the setting.
// (K2s takes its switches as a template argument, VT_SDBG in its unit.)
#ifdef VT_BATCH_TIMING_EXPERIMENTS
#define VT_DBG(a, bit) ((a).debug & (bit))
#else
#define VT_DBG(a, bit) false
#endif

namespace vt {
namespace dev {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// One LDS-DMA piece: 64 lanes x 16 B from (wave-uniform base + 32-bit lane offset) to LDS at lds_addr + lane * 16.
// Written out so that the address is the SGPR-base form (no 64-bit VALU add per piece) and the m0 write sits right in
// front of the load.  m0 is not listed as clobbered (the compiler reserves it); nothing else in these kernels uses it:
// gfx9+ LDS instructions do not, and there is no register-indexed access.
// NT: rows are read once (nt); a query image is re-read by every block (default policy).
// FENCE: the piece carries a "memory" clobber, so the compiler moves no LDS access across it.  K2 goes without:
// it places one piece per MFMA by hand between sched_barriers, every LDS read of a stage sits behind an s_waitcnt asm
// that carries the clobber and behind a barrier, and with the clobber its pieces and fragment reads move among the
// MFMAs (about 500 lines of the unit's assembly).
template <bool NT, bool FENCE = true>
__device__ __forceinline__ void dma16(uint32_t lds_addr, const void *base, uint32_t lane_off) {
  const uint64_t b = reinterpret_cast<uint64_t>(base);
  const uint64_t sb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t sl = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr);
  static_assert(FENCE || !NT, "the clobber-free form exists for K2's pieces alone");
  if (!FENCE) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(sl), "v"(lane_off), "s"(sb));
  else if (NT) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt" : : "s"(sl), "v"(lane_off), "s"(sb) : "memory");
  else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(sl), "v"(lane_off), "s"(sb) : "memory");
}

// Eight f32 to bf16, round to nearest even (v_cvt_pk_bf16_f32): the one rounding of every image and of K2b's rows.
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  const bf16x2 p0 = __builtin_convertvector((f32x2){lo[0], lo[1]}, bf16x2);
  const bf16x2 p1 = __builtin_convertvector((f32x2){lo[2], lo[3]}, bf16x2);
  const bf16x2 p2 = __builtin_convertvector((f32x2){hi[0], hi[1]}, bf16x2);
  const bf16x2 p3 = __builtin_convertvector((f32x2){hi[2], hi[3]}, bf16x2);
  bf16x8 o;
  o[0] = p0[0]; o[1] = p0[1]; o[2] = p1[0]; o[3] = p1[1];
  o[4] = p2[0]; o[5] = p2[1]; o[6] = p3[0]; o[7] = p3[1];
  return o;
}

// ---- the tile sequence ------------------------------------------------------------------------
// Block b of a grid of G takes tiles b, b + G, ... of `ntiles` (the caller has returned if b >= ntiles).
__device__ __forceinline__ uint32_t block_tiles(uint32_t ntiles) { return (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x; }
// The k-th of them as the sample counts it, and as a tile of the index: DENSE (the sample) takes every
// sample_stride-th tile.
__device__ __forceinline__ uint32_t sample_tile(uint32_t k) { return blockIdx.x + k * gridDim.x; }
template <bool DENSE>
__device__ __forceinline__ uint32_t index_tile(const BatchScoreArgs &a, uint32_t k) {
  return DENSE ? sample_tile(k) * a.sample_stride : sample_tile(k);
}

// The DMA cursor (tile dk of this block's, chunk dc) one chunk on; set_xsrc(dk) points the kernel's row source at a
// new tile.  Past the end of the sequence the cursor stays on the last chunk: the steady state keeps issuing (into a
// stage nobody reads any more) so that the loop body has no branches and the vmcnt arithmetic never changes.
template <class SetXsrc>
__device__ __forceinline__ void dma_advance(uint32_t &dk, uint32_t &dc, uint32_t nchunk, uint32_t my_tiles, SetXsrc &&set_xsrc) {
  if (dc + 1 == nchunk && dk + 1 == my_tiles) return;
  dc += 1;
  if (dc == nchunk) {
    dc = 0;
    dk += 1;
    set_xsrc(dk);
  }
}

// ---- accumulator layouts: the row that a lane's register holds, counted from the tile's first row row0 (the column
// is the lane's low bits), summed from row0 on, left to right, as the kernels always wrote it.
// 32x32 (K2, K2b): column = lane & 31, h = lane >> 5, register i of 16
__device__ __forceinline__ constexpr uint32_t c32_row(uint32_t row0, int i, int h) { return row0 + (i & 3) + 8 * (i >> 2) + 4 * h; }
// 16x16 (K2s): column = lane & 15, g = lane >> 4, register e of 4
__device__ __forceinline__ constexpr uint32_t c16_row(uint32_t row0, int g, int e) { return row0 + 4 * g + e; }

// ---- L2 family --------------------------------------------------------------------------------
// rank by s = 2 q.x - |x|^2 (larger s <=> smaller |q - x|^2)
__device__ __forceinline__ float l2_rank(float dot, float xnorm2) { return 2.0f * dot - xnorm2; }

// The row norms of a tile from its (wave-uniform) first row on, through the scalar cache (constant address space =>
// s_load): a vector load here would sit in the same in-order queue as the row DMA, and the wait for it would drain the
// ring once per tile.  The norm column is as long as the slab's row capacity, a multiple of 32: a run of 16 or 32 that
// starts below n_total at a multiple of its length ends inside it -- the caller asks only for such a row0.
typedef const __attribute__((address_space(4))) float *scalar_f32_p;
__device__ __forceinline__ scalar_f32_p scalar_norms(const BatchScoreArgs &a, uint32_t row0) {
  return (scalar_f32_p)(uintptr_t)(a.xnorm2 + row0);
}

// ---- filing -----------------------------------------------------------------------------------
// One (score, row) of query column qcol.  Premise 2 of the certificate in batch_group_finish lives here: every row
// < n_total whose score reaches tau is counted, past cand_cap too, and stored while the list has room.
__device__ __forceinline__ void file_candidate(const BatchScoreArgs &a, float s, float tau, uint32_t qcol, uint32_t row) {
  if (s >= tau && row < a.n_total) {
    const uint32_t pos = atomicAdd(&a.cand_count[qcol], 1u);
    if (pos < a.cand_cap) {
      BatchCand cnd;
      cnd.score = s;
      cnd.row = row;
      a.cand[(size_t)qcol * a.cand_cap + pos] = cnd;
    }
  }
}

// Cold path of an epilogue: some score of this lane's N (one query column) reaches the threshold; row_of(i) is the
// row register i holds -- a lambda that captures BY VALUE (with captures by reference K2's pass comes out with other
// registers and waits).  Inlined into its (rare) branch: as an out-of-line call it made the wave save and restore its
// live registers, 4 % of K2's pass.
// PIN: the list addresses are loop-invariant; hoisted out of the tile loop they cost 16 registers that K2b and K2s do
// not have -- behind the empty asm the compiler does not know where qcol comes from.
template <bool PIN, int N, class V, class RowOf>
__device__ __forceinline__ void append_candidates(const BatchScoreArgs &a, V v, float tau, uint32_t qcol, RowOf row_of) {
  if (PIN) asm volatile("" : "+v"(qcol));
#pragma unroll
  for (int i = 0; i < N; ++i) file_candidate(a, v[i], tau, qcol, row_of(i));
}

// ---- host side --------------------------------------------------------------------------------
// The launch's copy of the arguments: the product library runs no timing experiment, whatever the caller left in `debug`.
inline BatchScoreArgs batch_args_for_launch(const BatchScoreArgs &a0) {
  BatchScoreArgs a = a0;
#ifndef VT_BATCH_TIMING_EXPERIMENTS
  a.debug = 0u;
#endif
  return a;
}

}  // namespace dev
}  // namespace vt

// vt_prepare.hip -- K14 "prepare rows" (gfx950): what Collection.prepare_embedding does to a record's vector
// (collection.ex:921-946) for a whole matrix in one launch -- the finite check, one of the four normalizations
// (distances.rs:350-410) and the sign bits of the result (compress_sign_bits, :413-423).  The kernel is followed by its
// launcher.
//
// A wave takes kPrepWaveRows = 64 rows.  The reference's sums are serial f64 chains in index order, so lane l OWNS row l
// of the tile: it carries the row's accumulators from the first column to the last.  Global memory, however, is only
// ever touched with the lanes along the columns (one 256-byte run of a row per wave instruction).  Between the two
// stands a wave-private LDS image of one column panel, kPrepPanel = 64 columns of the 64 rows:
//
//   fill    for each row of the tile: lane c loads column c0 + c (coalesced) and files it at image[row][c];
//   chain   lane l walks image[l][0 .. 63] in column order: the finite check, then the mode's accumulators
//           (l2: acc += f64(x)^2; zscore: sum += f64(x); minmax: the in-order fminf / fmaxf fold);
//   zscore  walks the panels a second time for sum (f64(x) - mean)^2: the mean must be known first;
//   write   row by row, the lanes along the columns again: the row's scalars come from their owner by a lane read,
//           every lane converts, divides (a true f64 division), rounds and stores its own columns, and the ballot of
//           `result >= 0` over the 64 lanes IS the row's next sign word.  The words of the tile gather in lanes 0 .. 63
//           and leave 64 at a time as one contiguous store.
//
// The image's rows are kPrepPanel + 1 floats apart: the fill writes image[row][lane] (banks lane + row: distinct over
// a 32-lane group) and the chain reads image[lane][j] (banks 65 * lane + j = lane + j mod 32: distinct again), so
// neither side of the transpose meets a bank conflict (ds_read_b32 / ds_write_b32 bank = dword address mod 32 within
// each half wave).  Accumulators live in registers from panel to panel: d is unbounded, no row has to fit in LDS.
//
// A row with a non-finite value among its first d columns is left unwritten, values and words, and its index goes to
// *first_refused by atomicMin; every other row is written.  `out` may be `in` (ld_out == ld_in): every element is read
// and written by the same lane, after the row's chains are complete, and no two waves share a row.
#include "vt_common.cuh"

namespace vt {

using namespace dev;

namespace {

constexpr uint32_t kPrepLd = kPrepPanel + 1;  // floats between two rows of the LDS image (the bank-conflict pad)
static_assert(kPrepWaveRows == (uint32_t)kWave && kPrepPanel == (uint32_t)kWave, "one lane per row, one lane per panel column");

// `v >= 0.0` on the bit pattern (v is never NaN here): the sign bit clear, or a zero of either sign.  No float compare,
// so the answer for a subnormal result does not depend on the wave's denormal mode.
__device__ __forceinline__ bool sign_bit_of(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u >> 31) == 0 || (u << 1) == 0;
}

// Rows [row0, row0 + 64) x columns [c0, c0 + 64) into the wave's image.  Every load is unconditional, its row and column
// clamped into the matrix, and what it brings is filed as it is: a row past n holds a copy of the last row (its owner
// lane chains over it and never reports or writes anything), a column past d a copy of column d - 1 (the chain stops at
// d).  No load stands under a condition -- the compiler turns one into a branch, a branch ends the block its scheduler
// works in, and each of the 64 loads is then waited for on its own (measured: that form ran no faster with 64 loads
// "in flight" than with 16).  Straight-line, all 64 are issued before the first is filed; the block's LDS, not its
// registers, sets the occupancy.
__device__ __forceinline__ void fill_panel(const float *in, size_t ld_in, uint32_t n, uint32_t d, uint32_t row0,
                                           uint32_t c0, float *img, int lane) {
  const uint32_t col = c0 + (uint32_t)lane;
  const uint32_t last = (n - row0 < kPrepWaveRows ? n - row0 : kPrepWaveRows) - 1;  // (wave-uniform)
  const float *src = in + (size_t)row0 * ld_in + (col < d ? col : d - 1);
  float v[kPrepWaveRows];
#pragma unroll
  for (uint32_t r = 0; r < kPrepWaveRows; ++r) v[r] = src[(size_t)(r < last ? r : last) * ld_in];
#pragma unroll
  for (uint32_t r = 0; r < kPrepWaveRows; ++r) img[r * kPrepLd + lane] = v[r];
}

template <int MODE, bool WORDS>
__global__ __launch_bounds__(kPrepBlockRows) void prepare_rows_kernel(const PrepareArgs a) {
  __shared__ float s_img[kPrepBlockRows / kPrepWaveRows][kPrepWaveRows * kPrepLd];
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t wib = threadIdx.x >> 6;
  const uint64_t tile = (uint64_t)blockIdx.x * (kPrepBlockRows / kPrepWaveRows) + wib;
  if (tile * kPrepWaveRows >= a.n) return;  // (wave-uniform; the waves of a block never wait for each other)
  const uint32_t row0 = (uint32_t)(tile * kPrepWaveRows);
  const uint32_t n = a.n, d = a.d;
  float *img = s_img[wib];
  const float *mine = img + lane * kPrepLd;

  // ---- chain 1: the finite check and the mode's first accumulators, lane = row
  bool bad = false;
  double acc = 0.0;                          // l2: sum x^2; zscore: sum x
  float lo = INFINITY, hi = -INFINITY;       // minmax
  for (uint32_t c0 = 0; c0 < d; c0 += kPrepPanel) {
    fill_panel(a.in, a.ld_in, n, d, row0, c0, img, lane);
    wave_lds_fence();
    const uint32_t cols = d - c0 < kPrepPanel ? d - c0 : kPrepPanel;
    for (uint32_t j = 0; j < cols; ++j) {
      const float x = mine[j];
      bad |= !finite_f32(x);
      if (MODE == kPrepL2) {
        const double v = (double)x;
        acc += v * v;
      } else if (MODE == kPrepZscore) {
        acc += (double)x;
      } else if (MODE == kPrepMinmax) {
        // Rust's f32::min / max leave open which zero wins between +0.0 and -0.0, and so do fminf / fmaxf: a row whose
        // minimum is a zero and that holds zeros of both signs may get the other sign on a zero result.  UNPINNED.
        lo = fminf(lo, x);
        hi = fmaxf(hi, x);
      }
    }
    wave_lds_fence();  // (the next fill overwrites what this chain read)
  }

  // ---- the row's scalars: y = (f64(x) - sub) / div, or zeros
  double sub = 0.0, div = 1.0;
  bool zero = false;
  if (MODE == kPrepL2) {
    div = sqrt(acc);
    zero = div == 0.0;
  } else if (MODE == kPrepZscore) {
    const double mean = acc / (double)d;
    // chain 2: sum (x - mean)^2 over the same panels, read again (a refused row's chain runs on garbage, unused)
    double var = 0.0;
    for (uint32_t c0 = 0; c0 < d; c0 += kPrepPanel) {
      fill_panel(a.in, a.ld_in, n, d, row0, c0, img, lane);
      wave_lds_fence();
      const uint32_t cols = d - c0 < kPrepPanel ? d - c0 : kPrepPanel;
      for (uint32_t j = 0; j < cols; ++j) {
        const double diff = (double)mine[j] - mean;
        var += diff * diff;
      }
      wave_lds_fence();
    }
    sub = mean;
    div = sqrt(var / (double)d);
    zero = div == 0.0;
  } else if (MODE == kPrepMinmax) {
    sub = (double)lo;
    div = (double)hi - (double)lo;
    zero = lo == hi;
  }
  if (bad && row0 + (uint32_t)lane < n) atomicMin(a.first_refused, row0 + (uint32_t)lane);

  // ---- write: lanes along the columns, the owner's scalars broadcast.  The tile's (row, 64-column run) pairs are walked
  // kPrepInFlight at a time -- all loads of a batch first, then the arithmetic and the stores -- because `out` may be
  // `in`: the compiler may not move a load above a store on its own.  Pair u of the tile owns word u of the tile's words
  // (they are contiguous: [row][W]); lane u % 64 keeps it until 64 are gathered.
  const uint32_t rows = n - row0 < kPrepWaveRows ? n - row0 : kPrepWaveRows;
  const uint32_t W = (d + 63) / 64;
  const uint32_t total = rows * W;  // (rows <= 64, W <= 2^25)
  uint64_t word = 0;
  bool word_live = false;
  uint32_t r = 0, wi = 0;  // pair u0's row of the tile and run of the row (wave-uniform)
  for (uint32_t u0 = 0; u0 < total; u0 += kPrepInFlight) {
    float v[kPrepInFlight];
    uint32_t lr = r, lw = wi;  // the loads' own cursor: the second loop walks the same pairs again
#pragma unroll
    for (int k = 0; k < kPrepInFlight; ++k) {
      // (unconditional and clamped into the matrix, as in fill_panel: what a refused row or a pair past the tile's last
      // one loads is never used)
      const uint32_t j = lw * 64 + (uint32_t)lane;
      v[k] = a.in[((size_t)row0 + (lr < rows ? lr : rows - 1)) * a.ld_in + (j < d ? j : d - 1)];
      if (++lw == W) {
        lw = 0;
        ++lr;
      }
    }
#pragma unroll
    for (int k = 0; k < kPrepInFlight; ++k) {
      const uint32_t u = u0 + k;
      if (u >= total) break;  // (wave-uniform)
      const bool live = __shfl((int)bad, (int)r) == 0;
      bool bit = false;
      if (live) {
        const uint32_t j = wi * 64 + (uint32_t)lane;
        float y = v[k];
        if (MODE != kPrepNone) {
          const bool r_zero = __shfl((int)zero, (int)r) != 0;
          const double r_sub = __shfl(sub, (int)r), r_div = __shfl(div, (int)r);
          y = r_zero ? 0.0f : (float)(((double)y - r_sub) / r_div);
        }
        if (j < d) {
          a.out[((size_t)row0 + r) * a.ld_out + j] = y;
          bit = sign_bit_of(y);
        }
      }
      if (WORDS) {
        const uint64_t m = __ballot(bit);
        if ((u & 63u) == (uint32_t)lane) {
          word = m;
          word_live = live;
        }
        if ((u & 63u) == 63u || u + 1 == total) {  // 64 words gathered, or the tile's last one
          const uint32_t base = u & ~63u;
          if (base + (uint32_t)lane <= u && word_live) a.words[(size_t)row0 * W + base + lane] = word;
        }
      }
      if (++wi == W) {
        wi = 0;
        ++r;
      }
    }
  }
}

template <int MODE>
hipError_t launch_mode(const PrepareArgs &a, hipStream_t s) {
  const uint32_t blocks = (uint32_t)(((uint64_t)a.n + kPrepBlockRows - 1) / kPrepBlockRows);
  if (a.words)
    hipLaunchKernelGGL((prepare_rows_kernel<MODE, true>), dim3(blocks), dim3(kPrepBlockRows), 0, s, a);
  else
    hipLaunchKernelGGL((prepare_rows_kernel<MODE, false>), dim3(blocks), dim3(kPrepBlockRows), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_prepare_rows(const PrepareArgs &a, int mode, hipStream_t s) {
  if (mode < kPrepNone || mode > kPrepMinmax || !a.first_refused) return hipErrorInvalidValue;
  if (a.n == 0 || a.d == 0) return hipSuccess;
  if (!a.in || !a.out || a.ld_in < a.d || a.ld_out < a.d) return hipErrorInvalidValue;
  switch (mode) {
    case kPrepNone: return launch_mode<kPrepNone>(a, s);
    case kPrepL2: return launch_mode<kPrepL2>(a, s);
    case kPrepZscore: return launch_mode<kPrepZscore>(a, s);
    default: return launch_mode<kPrepMinmax>(a, s);
  }
}

}  // namespace vt

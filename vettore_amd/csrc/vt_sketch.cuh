// vt_sketch.cuh -- what the sketch units share (vt_sketch.hip: K1q, the int8 sketch's builders, the tail and the kernels
// behind the nibble passes; vt_sketch_batch.hip: K1qm; vt_sketch_nibble.hip, through vt_sketch_nibble.cuh: the builders and
// passes of K1s, K1f and K1n): the 16-byte vector type, wave reductions, the outward f64 -> f32 roundings of the bounds and
// their slack.
#pragma once
#include "vt_scan.cuh"

namespace vt {
namespace {

using namespace dev;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, kWave);
  return v;
}

// f64 -> f32 rounded towards +inf / -inf (finite inputs)
__device__ __forceinline__ float f32_up(double v) {
  const float f = (float)v;
  return (double)f < v ? nextafterf(f, INFINITY) : f;
}
__device__ __forceinline__ float f32_down(double v) {
  const float f = (float)v;
  return (double)f > v ? nextafterf(f, -INFINITY) : f;
}
constexpr double kSlack = 1.0 + 0x1p-40;  // covers the f64 rounding of the bound's own arithmetic

}  // namespace
}  // namespace vt

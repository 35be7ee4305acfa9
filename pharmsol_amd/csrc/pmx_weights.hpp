// pmx_weights.hpp — what the reductions over the support points share (pmx_posterior.hip, pmx_exposure.hip): the weight
// q of one column and the fixed-order sums over an item's owner.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pmx {
namespace {

__device__ __forceinline__ double neg_inf() { return -__builtin_inf(); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// q of one column; `bad`: a weight that is negative or NaN, or a q that is NaN
__device__ __forceinline__ double q_of(double wp, double x, double lp, bool posterior, bool& bad) {
  double q = 0.0;
  if (wp > 0.0) q = !posterior ? wp : (x == neg_inf() ? 0.0 : wp * exp(x - lp));
  bad = bad || !(wp >= 0.0) || q != q;
  return q;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  return x;  // (the same bits in every lane: each stage adds the same two numbers on both sides)
}

// The sum over the item's owner, in every thread of it.  Block-owned: the waves' sums meet in LDS and are added in wave
// order; two buffers in turn, so that one barrier per sum is enough (a thread that writes buffer b again has passed the
// barrier of the sum in between, which every thread reaches only after it has read b).
template <int WAVES>
__device__ __forceinline__ double owner_sum(double x, double (*sh)[4], int& turn, int lane, int wave) {
  x = wave_sum(x);
  if constexpr (WAVES > 1) {
    if (lane == 0) sh[turn][wave] = x;
    __syncthreads();
    x = ((sh[turn][0] + sh[turn][1]) + sh[turn][2]) + sh[turn][3];
    turn ^= 1;
  }
  return x;
}

}  // namespace
}  // namespace pmx

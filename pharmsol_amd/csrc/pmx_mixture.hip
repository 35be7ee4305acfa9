// pmx_mixture.hip — the two reductions NPAG / NPOD take of the log-likelihood matrix ll[n_subjects][ld] that
// pmx_loglik_device wrote, so that the matrix never has to leave the device:
//
//   pmx_mixture_rows     lpyl[s] = ln sum_{p: w[p] > 0} w[p] exp(ll[s][p])         (the mixture log-likelihood per subject)
//   pmx_dfunction_cols   slab[t][p] = sum_{s in tile t} exp(ll[s][p] - lpyl[s])    (partial column sums, one row per tile)
//   pmx_dfunction_sum    D[p] = sum_t slab[t][p] - n_subjects                      (ParameterOptimizer::cost returns -D)
//
// Both are read-bound: ll is read once, 8 bytes per lane and 512 contiguous bytes per wave instruction (ll is only
// 8-byte aligned with any ld >= n_support, include/pmx.h; nothing wider is loaded, so no row needs its alignment
// proven), and a vector comes out.  Everything is summed in a fixed order - a lane's strided elements, then an xor
// butterfly, then waves through LDS resp. tiles in a second launch; no float atomics, no hand-off between workgroups
// inside a launch (an atomic sum depends on arrival order; a hand-off needs an agent-scope release and an acquire in
// every consumer, and a resident grid) - so a result does not depend on dispatch order and is bit-identical from run
// to run, for any base address and any ld.  Measurements and the variants tried: profiles/mixture_reductions.txt.
//
// Sharding by subjects needs nothing more: a rank's D subtracts the rank's own subject count, so the ranks' D vectors
// simply add (and the ranks' lpyl vectors concatenate).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmx_kernels.hpp"

namespace pmx {
namespace {

__device__ __forceinline__ double neg_inf() { return -__builtin_inf(); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// A running (max, sum scaled by exp(-max)) pair takes four more terms w exp(x) at once: the new maximum first, one
// rescaling of the sum, then four exps that do not wait for each other (one term at a time makes every exp wait for
// the maximum the term before it left: 16 in a row per lane at C3 size).  ok[k]: the term counts (in range, w > 0,
// x > -inf).  A NaN x leaves the maximum alone (fmax) and poisons the sum.
__device__ __forceinline__ void mix_add4(double& m, double& s, const double (&x)[4], const double (&w)[4], const bool (&ok)[4]) {
  double mn = m;
#pragma unroll
  for (int k = 0; k < 4; ++k) mn = ok[k] ? fmax(mn, x[k]) : mn;
  s = (m == mn) ? s : s * exp(m - mn);  // (equal also when both are -inf: inf - inf is NaN)
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (ok[k]) s = fma(w[k], (x[k] == mn) ? 1.0 : exp(x[k] - mn), s);
  m = mn;
}

// ... and two pairs become one (the four waves of a block-owned row, in wave order)
__device__ __forceinline__ void mix_merge(double& m, double& s, double m2, double s2) {
  const double e = (m == m2) ? 1.0 : exp(-fabs(m - m2));  // (an empty pair has max -inf and sum 0, or NaN: 0 * 0, NaN * 0)
  const bool keep = m >= m2;
  s = keep ? fma(s2, e, s) : fma(s, e, s2);
  m = keep ? m : m2;
}

// WAVES = 1: a wave owns a row, four rows per block; WAVES = 4: the block owns a row
template <int WAVES>
__global__ __launch_bounds__(256) void pmx_mixture_rows(const double* __restrict__ ll, int64_t S, int64_t P, int64_t ld,
                                                       const double* __restrict__ w, double* __restrict__ lpyl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = WAVES == 1 ? static_cast<int64_t>(blockIdx.x) * 4 + wave : static_cast<int64_t>(blockIdx.x);
  double m = neg_inf(), s = 0.0;
  if (row < S) {
    const double* __restrict__ r = ll + row * ld;
    constexpr int L = 64 * WAVES;  // lanes that share the row
    for (int64_t p0 = WAVES == 1 ? lane : static_cast<int>(threadIdx.x); p0 < P; p0 += 4 * L) {
      double x[4], wp[4];
      bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t p = p0 + k * L;
        const bool in = p < P;
        wp[k] = in ? w[p] : 0.0;
        x[k] = in ? r[p] : 0.0;
        if (!(wp[k] >= 0.0)) s = quiet_nan();  // a negative or NaN weight: the device form cannot refuse after the fact
        ok[k] = wp[k] > 0.0 && x[k] != neg_inf();  // a column without weight is skipped whatever it holds; -inf adds 0
      }
      mix_add4(m, s, x, wp, ok);
    }
  }
  // across the wave: the maximum first (no exp), ONE rescaling per lane, then plain sums - six merges of pairs would
  // cost six exps per lane, more than the lane's own elements at C3 size
  double wm = m;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) wm = fmax(wm, __shfl_xor(wm, off));  // (a lane's maximum is never NaN)
  s = (m == wm) ? s : s * exp(m - wm);  // an empty lane under a finite maximum: 0 * 0, or NaN * 0
  m = wm;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if constexpr (WAVES == 1) {
    if (lane == 0 && row < S) lpyl[row] = m + log(s);  // all -inf: -inf + ln 0
  } else {
    __shared__ double sh_m[4], sh_s[4];
    if (lane == 0) {
      sh_m[wave] = m;
      sh_s[wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // (the grid has exactly S blocks)
      for (int k = 1; k < 4; ++k) mix_merge(m, s, sh_m[k], sh_s[k]);
      lpyl[row] = m + log(s);
    }
  }
}

// One wave = one tile of rows x up to 64 columns; the four waves of a block take four neighbouring tiles.
// SMALL (n_cand <= 32): a wave's lanes are (64 >> cshift) rows x (1 << cshift) columns, so that n_cand = 1 - the
// reference's own call shape - still reads 64 rows per instruction; the rows of a column meet in an xor butterfly.
// Otherwise lanes run along the columns and lpyl[s] is wave-uniform.
template <bool SMALL>
__global__ __launch_bounds__(256) void pmx_dfunction_cols(const double* __restrict__ ll, int64_t S, int64_t P, int64_t ld,
                                                         const double* __restrict__ lpyl, double* __restrict__ slab,
                                                         int cshift, int64_t n_tiles) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t tile = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  if (tile >= n_tiles) return;  // (wave-uniform)
  const int r = SMALL ? lane >> cshift : 0;            // the lane's row within a pass
  const int rows_per_pass = SMALL ? 64 >> cshift : 1;
  const int64_t col = SMALL ? static_cast<int64_t>(lane & ((1 << cshift) - 1)) : static_cast<int64_t>(blockIdx.y) * 64 + lane;
  const int64_t s0 = tile * kDfunctionPasses * rows_per_pass;
  const int64_t s1 = s0 + kDfunctionPasses * rows_per_pass < S ? s0 + kDfunctionPasses * rows_per_pass : S;
  double acc = 0.0;
  if (col < P) {
#pragma unroll 4
    for (int64_t s = s0 + r; s < s1; s += rows_per_pass) acc += exp(ll[s * ld + col] - lpyl[s]);
  }
  if constexpr (SMALL) {
    for (int off = 32; off >= (1 << cshift); off >>= 1) acc += __shfl_xor(acc, off);
  }
  if (col < P && r == 0) slab[tile * P + col] = acc;
}

// the slabs added in tile order, one lane per column
__global__ __launch_bounds__(64) void pmx_dfunction_sum(const double* __restrict__ slab, int64_t n_tiles, int64_t P,
                                                       double n_subjects, double* __restrict__ D) {
  const int64_t col = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
  if (col >= P) return;
  double acc = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < n_tiles; ++t) acc += slab[t * P + col];
  D[col] = acc - n_subjects;
}

}  // namespace

hipError_t launch_mixture_rows(const double* d_ll, int64_t S, int64_t P, int64_t ld, const double* d_w, double* d_lpyl,
                               void* stream) {
  if (S <= 0) return hipSuccess;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool block_per_row = P > kMixtureWaveRowMax;
  const int64_t blocks = block_per_row ? S : (S + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 g(static_cast<uint32_t>(blocks)), b(256);
  if (block_per_row)
    hipLaunchKernelGGL(pmx_mixture_rows<4>, g, b, 0, st, d_ll, S, P, ld, d_w, d_lpyl);
  else
    hipLaunchKernelGGL(pmx_mixture_rows<1>, g, b, 0, st, d_ll, S, P, ld, d_w, d_lpyl);
  return hipGetLastError();
}

hipError_t launch_dfunction(const double* d_ll, int64_t S, int64_t n_cand, int64_t ld, const double* d_lpyl,
                            double* d_scratch, double* d_D, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_tiles = S > 0 ? dfunction_tiles(S, n_cand) : 0;
  if (n_tiles > 0) {
    const int cshift = dfunction_cshift(n_cand);
    const int64_t groups = cshift < 6 ? 1 : (n_cand + 63) / 64, blocks = (n_tiles + 3) / 4;
    if (blocks > 0x7fffffff || groups > 65535) return hipErrorInvalidValue;
    const dim3 g(static_cast<uint32_t>(blocks), static_cast<uint32_t>(groups)), b(256);
    if (cshift < 6)
      hipLaunchKernelGGL(pmx_dfunction_cols<true>, g, b, 0, st, d_ll, S, n_cand, ld, d_lpyl, d_scratch, cshift, n_tiles);
    else
      hipLaunchKernelGGL(pmx_dfunction_cols<false>, g, b, 0, st, d_ll, S, n_cand, ld, d_lpyl, d_scratch, cshift, n_tiles);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pmx_dfunction_sum, dim3(static_cast<uint32_t>((n_cand + 63) / 64)), dim3(64), 0, st, d_scratch, n_tiles,
                     n_cand, static_cast<double>(S), d_D);
  return hipGetLastError();
}

}  // namespace pmx

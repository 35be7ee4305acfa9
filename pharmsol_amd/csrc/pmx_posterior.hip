// pmx_posterior.hip — what a fit reports of the prediction matrix pred[n_obs][ld] that pmx_predict_device wrote, reduced
// where the matrix is:
//
//   pmx_posterior_rows   q[s][p] = w[p] exp(ll[s][p] - lpyl[s])   (w[p] > 0; else 0)   the posterior of subject s
//   pmx_summary_rows     mean[row]   = sum_p q pred[row][p] / sum_p q                   over the columns with q > 0
//                        median[row] = the smallest pred[row][p], q > 0, with sum_{p': pred[row][p'] <= v} q >= sum_p q / 2
//                        q = the posterior of the row's subject (MODE posterior) or w itself (MODE population)
//
// A work item is up to rows_per_item consecutive rows - of ONE subject in posterior mode - and belongs to a wave (up to
// 1024 columns, four items per block) or to a block of four waves.  The owner forms the item's q once (one exp per
// column) and keeps it in registers, NQ per lane, column k * lanes + lane in slot k; then it walks the rows: 8-byte loads
// strided by lane (512 contiguous bytes per wave instruction, no alignment to prove), the products summed over a lane's
// slots in slot order, then an xor butterfly, then - block-owned items - the four waves through LDS in wave order.  No
// float atomics and no hand-off between workgroups, so a result depends on neither dispatch order nor addresses: it is
// bit-identical from run to run, for any base alignment and any ld.
//
// The median is a selection, not a sort: the doubles map to 64-bit keys in their order (sign bit flipped for positive
// values, all bits for negative ones), and the answer's key is built from the top bit down - a round adds the weight
// below the trial key in the same fixed order and keeps the bit if that weight is still short of half the total.  The
// masked sums are monotone in the trial key (the same non-negative terms in the same order), so the rounds are
// consistent among themselves, and the key they end at is a key of the row: the value comes back bit for bit.  The row's
// keys stay in registers for the 64 rounds.  Rows wider than 4096 columns do not fit: NQ = 0 recomputes q and re-reads
// the row in every round - correct for any P, and slow.
//
// Edges (include/pmx.h): a column with w == 0 is skipped whatever ll and pred hold there; ll = -inf gives q = 0; a
// negative or NaN weight gives NaN everywhere; a NaN q (a failed pair under weight) gives NaN in all rows of that subject
// and in no other; a NaN prediction under q > 0 gives NaN in that row; a row whose q are all 0 gives NaN.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmx_kernels.hpp"
#include "pmx_weights.hpp"  // q_of, wave_sum, owner_sum: shared with pmx_exposure.hip

namespace pmx {
namespace {

__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// the doubles in their order as unsigned integers (-0.0 just below +0.0; NaNs at the two ends, never selected)
__device__ __forceinline__ uint64_t key_of(double v) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(v));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  return __longlong_as_double(static_cast<long long>((k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k));
}

struct SummaryParams {
  const double* __restrict__ pred;
  int64_t n_obs, P, ld_pred;
  const double* __restrict__ w;
  const double* __restrict__ ll;
  int64_t ld_ll;
  const double* __restrict__ lpyl;
  const int64_t* __restrict__ subj_obs_off;
  int64_t n_items, rows_per_item;
  double* __restrict__ mean;
  double* __restrict__ median;
};

// WAVES = 1: a wave owns an item, four items per block; WAVES = 4: the block owns one.  NQ > 0: columns per lane kept in
// registers (P <= 64 WAVES NQ); NQ = 0: any P, nothing kept.  MEDIAN: the median too (the mean where a.mean is given).
template <int WAVES, int NQ, bool POSTERIOR, bool MEDIAN>
__global__ __launch_bounds__(256) void pmx_summary_rows(const SummaryParams a) {
  constexpr int L = 64 * WAVES;    // lanes that share the item
  constexpr int NR = NQ > 0 ? NQ : 1;
  __shared__ double sh[2][4];
  int turn = 0;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int t = WAVES == 1 ? lane : static_cast<int>(threadIdx.x);
  const int64_t item = WAVES == 1 ? static_cast<int64_t>(blockIdx.x) * 4 + wave : static_cast<int64_t>(blockIdx.x);
  if (item >= a.n_items) return;  // (uniform over the owner; a wave-owned item meets no barrier)
  int64_t r0, r1;
  const double* __restrict__ llrow = nullptr;
  double lp = 0.0;
  if constexpr (POSTERIOR) {
    const int64_t o0 = a.subj_obs_off[item], o1 = a.subj_obs_off[item + 1];
    r0 = o0 + static_cast<int64_t>(blockIdx.y) * a.rows_per_item;
    r1 = r0 + a.rows_per_item < o1 ? r0 + a.rows_per_item : o1;
    llrow = a.ll + item * a.ld_ll;
    lp = a.lpyl[item];
  } else {
    r0 = item * a.rows_per_item;
    r1 = r0 + a.rows_per_item < a.n_obs ? r0 + a.rows_per_item : a.n_obs;
  }
  r0 = uniform64(r0);
  r1 = uniform64(r1);
  if (r0 >= r1) return;

  // the item's q: once, into registers (NQ > 0), or summed here and formed again wherever it is used (NQ = 0)
  double q[NR];
  bool bad = false;
  double den = 0.0;
  if constexpr (NQ > 0) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const int64_t p = static_cast<int64_t>(k) * L + t;
      const bool in = p < a.P;
      const double wp = in ? a.w[p] : 0.0;
      const double x = (POSTERIOR && in) ? llrow[p] : 0.0;
      q[k] = q_of(wp, x, lp, POSTERIOR, bad);
      den += q[k];
    }
  } else {
    for (int64_t p = t; p < a.P; p += L) den += q_of(a.w[p], POSTERIOR ? llrow[p] : 0.0, lp, POSTERIOR, bad);
  }
  den = owner_sum<WAVES>(den, sh, turn, lane, wave);
  bad = owner_sum<WAVES>(bad ? 1.0 : 0.0, sh, turn, lane, wave) > 0.0 || !(den > 0.0);  // (no column with q > 0: NaN too)
  const double half = 0.5 * den;

  for (int64_t r = r0; r < r1; ++r) {
    const double* __restrict__ row = a.pred + r * a.ld_pred;
    uint64_t key[NR];
    double num = 0.0;
    bool nan_seen = false;
    if constexpr (NQ > 0) {
      double v[NQ];
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const int64_t p = static_cast<int64_t>(k) * L + t;
        v[k] = p < a.P ? row[p] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        if (q[k] > 0.0) {
          num = fma(q[k], v[k], num);
          nan_seen = nan_seen || v[k] != v[k];
        }
        key[k] = key_of(v[k]);
      }
    } else {
      bool b2 = false;
      for (int64_t p = t; p < a.P; p += L) {
        const double qp = q_of(a.w[p], POSTERIOR ? llrow[p] : 0.0, lp, POSTERIOR, b2);
        const double v = row[p];
        if (qp > 0.0) {
          num = fma(qp, v, num);
          nan_seen = nan_seen || v != v;
        }
      }
    }
    num = owner_sum<WAVES>(num, sh, turn, lane, wave);
    double med = 0.0;
    if constexpr (MEDIAN) {
      nan_seen = owner_sum<WAVES>(nan_seen ? 1.0 : 0.0, sh, turn, lane, wave) > 0.0;
      uint64_t ans = 0;
      for (int bit = 63; bit >= 0; --bit) {
        const uint64_t trial = ans | (uint64_t{1} << bit);
        double below = 0.0;
        if constexpr (NQ > 0) {
#pragma unroll
          for (int k = 0; k < NQ; ++k) below += key[k] < trial ? q[k] : 0.0;  // (q is 0 in every column that does not count)
        } else {
          bool b2 = false;
          for (int64_t p = t; p < a.P; p += L) {
            const double qp = q_of(a.w[p], POSTERIOR ? llrow[p] : 0.0, lp, POSTERIOR, b2);
            below += (qp > 0.0 && key_of(row[p]) < trial) ? qp : 0.0;
          }
        }
        below = owner_sum<WAVES>(below, sh, turn, lane, wave);
        // every lane holds the same sum: the answer so far lives in scalar registers
        ans = static_cast<uint64_t>(uniform64(static_cast<int64_t>(below < half ? trial : ans)));
      }
      med = nan_seen ? quiet_nan() : value_of(ans);
    }
    if (t == 0) {
      if (a.mean != nullptr) a.mean[r] = bad ? quiet_nan() : num / den;
      if constexpr (MEDIAN) a.median[r] = bad ? quiet_nan() : med;
    }
  }
}

// a wave owns a row of ll, four rows per block: the weights are looked through first (a bad one anywhere makes the
// whole row NaN), then one exp and one 8-byte store per column
__global__ __launch_bounds__(256) void pmx_posterior_rows(const double* __restrict__ ll, int64_t S, int64_t P, int64_t ld_ll,
                                                         const double* __restrict__ w, const double* __restrict__ lpyl,
                                                         double* __restrict__ post, int64_t ld_post) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  if (s >= S) return;
  bool bad_w = false;
  for (int64_t p = lane; p < P; p += 64) bad_w = bad_w || !(w[p] >= 0.0);
  bad_w = __any(bad_w);
  const double* __restrict__ r = ll + s * ld_ll;
  double* __restrict__ o = post + s * ld_post;
  const double lp = lpyl[s];
#pragma unroll 4
  for (int64_t p = lane; p < P; p += 64) {
    bool bad = false;
    const double q = q_of(w[p], r[p], lp, true, bad);
    o[p] = bad_w ? quiet_nan() : q;  // (a NaN q is stored as it is: that column, that subject)
  }
}

template <int WAVES, int NQ>
hipError_t launch_summary_as(const SummaryParams& p, dim3 g, hipStream_t st, bool posterior, bool median) {
  return dispatch(
      [&](auto post, auto med) {
        hipLaunchKernelGGL((pmx_summary_rows<WAVES, NQ, decltype(post)::value, decltype(med)::value>), g, dim3(256), 0, st, p);
        return hipGetLastError();
      },
      posterior, median);
}

}  // namespace

hipError_t launch_posterior_rows(const double* d_ll, int64_t S, int64_t P, int64_t ld_ll, const double* d_w,
                                 const double* d_lpyl, double* d_post, int64_t ld_post, void* stream) {
  if (S <= 0) return hipSuccess;
  const int64_t blocks = (S + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pmx_posterior_rows, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     d_ll, S, P, ld_ll, d_w, d_lpyl, d_post, ld_post);
  return hipGetLastError();
}

hipError_t launch_summary_rows(const SummaryArgs& a, void* stream) {
  if (a.n_obs <= 0) return hipSuccess;
  const bool posterior = a.ll != nullptr;
  if (posterior && (a.S <= 0 || a.max_subject_rows <= 0)) return hipSuccess;
  SummaryParams p{a.pred, a.n_obs, a.P, a.ld_pred, a.w, a.ll, a.ld_ll, a.lpyl, a.subj_obs_off, 0, kSummaryRowsPerItem,
                  a.mean, a.median};
  int64_t gy = 1;
  if (posterior) {  // items: subjects x chunks of a subject's rows (grid.y; at most 65535 of them)
    p.n_items = a.S;
    if ((a.max_subject_rows + p.rows_per_item - 1) / p.rows_per_item > 65535) p.rows_per_item = (a.max_subject_rows + 65534) / 65535;
    gy = (a.max_subject_rows + p.rows_per_item - 1) / p.rows_per_item;
  } else {
    p.n_items = (a.n_obs + p.rows_per_item - 1) / p.rows_per_item;
  }
  const bool wave_owned = a.P <= kSummaryWaveMax;
  const int64_t blocks = wave_owned ? (p.n_items + 3) / 4 : p.n_items;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 g(static_cast<uint32_t>(blocks), static_cast<uint32_t>(gy));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool median = a.median != nullptr;
  if (a.P <= 64) return launch_summary_as<1, 1>(p, g, st, posterior, median);
  if (a.P <= 256) return launch_summary_as<1, 4>(p, g, st, posterior, median);
  if (wave_owned) return launch_summary_as<1, 16>(p, g, st, posterior, median);
  if (a.P <= kSummaryRegisterMax) return launch_summary_as<4, 16>(p, g, st, posterior, median);
  return launch_summary_as<4, 0>(p, g, st, posterior, median);
}

}  // namespace pmx

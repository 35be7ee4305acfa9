// pmx_exposure.hip — what a simulation takes of the prediction matrix pred[n_obs][ld] that pmx_predict_device wrote,
// reduced where the matrix is (the arithmetic, stated once: include/pmx.h):
//
//   pmx_exposure_rows     per (profile, support point): AUC, AUMC, Cmax, Tmax, Cmin and the time above a threshold of the
//                         profile clipped to the window [a, b]; one plane [n_profiles][ld_out] per requested metric
//   pmx_attainment_rows   per profile: pta = sum_{q > 0, m >= target} q / sum q and mean = sum q m / sum q over the
//                         support points, q = w itself or the posterior of the profile's subject (q_of, pmx_weights.hpp)
//
// Exposure.  A profile is the prediction rows of one (subject, occasion, output equation); the population's profile table
// gives, in profile order, the row index and the time of every row.  The block-to-profile map: the work items are the
// pairs (profile, tile of 64 consecutive columns), the column tile fastest; wave w of block b owns item 4 b + w, lane l of
// it column 64 tile + l.  So a block is four waves that each walk their own profile rows - a profile of one row occupies
// a wave exactly as long as it takes -, the four waves of a block read 2 KiB of a row side by side when the matrix is
// at least 256 columns wide, and a matrix of up to 64 columns puts four profiles into a block.  No item count is a
// threshold: the only switch is the quotient item / tiles, taken in 32 bits while the item count fits them.
//
// The wave walks the rows of its profile serially.  Row index and row time are the same in all lanes: they are read
// through constant-address-space pointers, by the scalar unit, and everything that depends on times alone - which points
// lie in the window, where it cuts a segment, whether two points of the clipped profile coincide - is decided there, once
// per wave.  A row's 64 columns are one 8-byte load per lane, 512 contiguous bytes per wave instruction, no alignment to
// prove; the loads run four rows ahead of the arithmetic through a rotating set of registers.  Every element of pred is
// loaded exactly once, whatever the method and the set of metrics.  The running values - the previous point, the sums,
// the extremes - stay in registers, and the requested planes are written once at the end.
//
// PMX_AUC_LIN_LOG in the same single pass.  A pair of the clipped profile is integrated linearly when it ends at or before
// tmax, the time of the first-occurrence maximum of the unclipped profile.  Beside the running sum T (log pieces where
// use_log_linear says so) the lane keeps L, the sum of the linear pieces of the same pairs in the same order; whenever
// the fold over the unclipped profile finds a new maximum - after the pairs that end at that point have been added - it
// sets T = L.  After the last reset T is the linear pieces up to tmax followed by the mixed ones, added in the order the
// reference adds them: the same bits as a pass that knew tmax beforehand, for any number of rows, with nothing kept and
// nothing read twice.  (A pair that ends at tmax's time without ending at tmax's point has zero length: AUC is NaN.)
//
// No float atomics, no hand-off between workgroups: each (profile, column) is one lane's own sum in row order, and each
// attainment is summed per lane in column order, then by an xor butterfly, then - rows wider than kAttainWaveMax, owned by
// a block - over the four waves in wave order.  Results are bit-identical from run to run, for any alignment and any ld.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmx_device.hpp"
#include "pmx_kernels.hpp"
#include "pmx_weights.hpp"

// the formulas as written: a product and a sum stay two roundings (the fma of the weighted mean is spelled out)
#pragma clang fp contract(off)

namespace pmx {
namespace {

// use_log_linear, data/auc.rs:28-30
__device__ __forceinline__ bool use_log_linear(double c1, double c2) {
  return c2 < c1 && c1 > 0.0 && c2 > 0.0 && fabs((c1 / c2) - 1.0) >= 1e-10;
}

// what a lane carries along its profile
struct Lane {
  double kc;                     // value of the last point of the clipped profile K
  double auc, aumc;              // running sums (PMX_AUC_LIN_LOG: T)
  double lauc, laumc;            // PMX_AUC_LIN_LOG: L, the linear pieces of the same pairs
  double cmax, tmax, cmin, above;
  double gmax;                   // PMX_AUC_LIN_LOG: the maximum of the unclipped profile so far
  bool nan;
};

// one pair (t1, s.kc) -> (t2, c2) of K; t1, t2, dt are wave-uniform, dt > 0 wherever the sums are asked for
template <int METHOD>
__device__ __forceinline__ void add_pair(Lane& s, double t1, double t2, double c2, uint32_t metrics, bool sums, double thr) {
  const double c1 = s.kc;
  const double dt = t2 - t1;
  if (sums) {
    const bool want_aumc = (metrics & PMX_EXPO_AUMC) != 0;
    const double lin_auc = (c1 + c2) / 2.0 * dt;                                   // auc_linear
    const double lin_aumc = want_aumc ? (t1 * c1 + t2 * c2) / 2.0 * dt : 0.0;      // aumc_linear
    double v_auc = lin_auc, v_aumc = lin_aumc;
    if constexpr (METHOD != PMX_AUC_LINEAR) {
      if (use_log_linear(c1, c2)) {
        const double r = log(c1 / c2);
        v_auc = (c1 - c2) * dt / r;                                                // auc_log
        if (want_aumc) {
          const double k = r / dt;
          v_aumc = (t1 * c1 - t2 * c2) / k + (c1 - c2) / (k * k);                  // aumc_log
        }
      }
    }
    s.auc += v_auc;
    s.aumc += v_aumc;
    if constexpr (METHOD == PMX_AUC_LIN_LOG) {
      s.lauc += lin_auc;
      s.laumc += lin_aumc;
    }
  }
  if (metrics & PMX_EXPO_TIME_ABOVE) {  // nca/calc.rs:719-737
    const bool up1 = c1 >= thr, up2 = c2 >= thr;
    double add = 0.0;
    if (up1 && up2) {
      add = dt;
    } else if (up1 && c2 < thr) {
      const double t_cross = t1 + dt * (c1 - thr) / (c1 - c2);
      add = t_cross - t1;
    } else if (c1 < thr && up2) {
      const double t_cross = t1 + dt * (thr - c1) / (c2 - c1);
      add = t2 - t_cross;
    }
    s.above += add;
  }
}

struct ExpoParams {
  const double* __restrict__ pred;
  int64_t P, ld_pred;
  const int64_t* __restrict__ prof_off;
  const int64_t* __restrict__ prof_row;
  const double* __restrict__ prof_time;
  int64_t n_profiles, n_ctiles, n_items;
  double a, b, threshold;
  uint32_t metrics;
  double* __restrict__ out;
  int64_t ld_out;
};

template <int METHOD>
__global__ __launch_bounds__(256) void pmx_exposure_rows(const ExpoParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t item = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  if (item >= p.n_items) return;
  int64_t prof;
  if (p.n_items <= 0xffffffffLL)
    prof = static_cast<int64_t>(static_cast<uint32_t>(item) / static_cast<uint32_t>(p.n_ctiles));
  else
    prof = item / p.n_ctiles;
  const int64_t col = (item - prof * p.n_ctiles) * 64 + lane;
  if (col >= p.P) return;  // (a lane's own exit: nothing below crosses lanes)
  const cptr<int64_t> rows = as_const(p.prof_row);
  const cptr<double> times = as_const(p.prof_time);
  const int64_t r0 = as_const(p.prof_off)[prof];
  const int64_t n = as_const(p.prof_off)[prof + 1] - r0;  // >= 1: only profiles with a row exist
  const double* __restrict__ base = p.pred + col;
  const uint32_t metrics = p.metrics;
  const bool want_sums = (metrics & (PMX_EXPO_AUC | PMX_EXPO_AUMC)) != 0;
  const double a = p.a, b = p.b, thr = p.threshold;

  Lane s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, neg_inf(), false};
  // wave-uniform: the points of K so far, the time of its last one, a zero-length pair among them
  int64_t kcount = 0;
  double kt = 0.0;
  bool zero_len = false;
  double tp = 0.0, cp = 0.0;  // the previous point of the unclipped profile (from the second row on)

  // the loads run four rows ahead
  double v0 = base[rows[r0] * p.ld_pred], v1 = 0.0, v2 = 0.0, v3 = 0.0;
  if (n > 1) v1 = base[rows[r0 + 1] * p.ld_pred];
  if (n > 2) v2 = base[rows[r0 + 2] * p.ld_pred];
  if (n > 3) v3 = base[rows[r0 + 3] * p.ld_pred];
  for (int64_t i = 0; i < n; ++i) {
    const double c = v0;
    v0 = v1;
    v1 = v2;
    v2 = v3;
    if (i + 4 < n) v3 = base[rows[r0 + i + 4] * p.ld_pred];
    const double t = times[r0 + i];
    s.nan = s.nan || c != c;
    // what this row adds to K, in order: the cut at a, the cut at b (both strictly inside the segment that ends here), the
    // point itself (never together with the cut at b)
#pragma nounroll
    for (int e = 0; e < 3; ++e) {
      const double te = e == 0 ? a : (e == 1 ? b : t);
      const bool on = e == 2 ? (a <= t && t <= b) : (i > 0 && tp < te && te < t);
      if (!on) continue;
      double ce = c;
      if (e != 2) ce = fabs(t - tp) < 1e-10 ? cp : cp + (c - cp) * (te - tp) / (t - tp);  // interpolate_linear, auc.rs:357-361
      if (kcount > 0) {
        const bool sums = want_sums && te - kt > 0.0;
        zero_len = zero_len || (want_sums && !sums);
        add_pair<METHOD>(s, kt, te, ce, metrics, sums, thr);
        if (ce > s.cmax) {
          s.cmax = ce;
          s.tmax = te;
        }
        if (ce < s.cmin) s.cmin = ce;
      } else {
        s.cmax = ce;
        s.tmax = te;
        s.cmin = ce;
      }
      ++kcount;
      kt = te;
      s.kc = ce;
    }
    if constexpr (METHOD == PMX_AUC_LIN_LOG) {
      if (c > s.gmax) {  // a new first-occurrence maximum: every pair so far ends at or before it
        s.gmax = c;
        s.auc = s.lauc;
        s.aumc = s.laumc;
      }
    }
    tp = t;
    cp = c;
  }

  const bool none = s.nan || kcount == 0;
  const bool no_pair = none || kcount < 2;
  const double nan = quiet_nan();
  double* __restrict__ o = p.out + prof * p.ld_out + col;
  const int64_t plane = p.n_profiles * p.ld_out;
  if (metrics & PMX_EXPO_AUC) {
    *o = (no_pair || zero_len) ? nan : s.auc;
    o += plane;
  }
  if (metrics & PMX_EXPO_AUMC) {
    *o = (no_pair || zero_len) ? nan : s.aumc;
    o += plane;
  }
  if (metrics & PMX_EXPO_CMAX) {
    *o = none ? nan : s.cmax;
    o += plane;
  }
  if (metrics & PMX_EXPO_TMAX) {
    *o = none ? nan : s.tmax;
    o += plane;
  }
  if (metrics & PMX_EXPO_CMIN) {
    *o = none ? nan : s.cmin;
    o += plane;
  }
  if (metrics & PMX_EXPO_TIME_ABOVE) *o = no_pair ? nan : s.above;
}

// WAVES = 1: a wave owns a profile's row of the metric plane, four rows per block; WAVES = 4: the block owns one.  A
// lane takes the columns t, t + L, ... in that order.
template <int WAVES, bool POSTERIOR>
__global__ __launch_bounds__(256) void pmx_attainment_rows(const AttainArgs a) {
  constexpr int L = 64 * WAVES;
  __shared__ double sh[2][4];
  int turn = 0;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int t = WAVES == 1 ? lane : static_cast<int>(threadIdx.x);
  const int64_t item = WAVES == 1 ? static_cast<int64_t>(blockIdx.x) * 4 + wave : static_cast<int64_t>(blockIdx.x);
  if (item >= a.n_profiles) return;  // (uniform over the owner; a wave-owned row meets no barrier)
  const double* __restrict__ row = a.metric + item * a.ld_metric;
  const double* __restrict__ llrow = nullptr;
  double lp = 0.0;
  if constexpr (POSTERIOR) {
    const int64_t subj = uniform64(a.prof_subject[item]);
    llrow = a.ll + subj * a.ld_ll;
    lp = a.lpyl[subj];
  }
  const double target = a.pta != nullptr ? a.target[item] : 0.0;
  double den = 0.0, num = 0.0, att = 0.0;
  bool bad = false, nan_seen = false;
  for (int64_t p = t; p < a.P; p += L) {
    const double q = q_of(a.w[p], POSTERIOR ? llrow[p] : 0.0, lp, POSTERIOR, bad);
    const double m = row[p];
    den += q;
    if (q > 0.0) {
      nan_seen = nan_seen || m != m;
      num = fma(q, m, num);
      att += m >= target ? q : 0.0;
    }
  }
  den = owner_sum<WAVES>(den, sh, turn, lane, wave);
  num = owner_sum<WAVES>(num, sh, turn, lane, wave);
  att = owner_sum<WAVES>(att, sh, turn, lane, wave);
  bad = owner_sum<WAVES>((bad || nan_seen) ? 1.0 : 0.0, sh, turn, lane, wave) > 0.0 || !(den > 0.0);  // (no column with q > 0: NaN too)
  if (t == 0) {
    if (a.pta != nullptr) a.pta[item] = bad ? quiet_nan() : att / den;
    if (a.mean != nullptr) a.mean[item] = bad ? quiet_nan() : num / den;
  }
}

template <int METHOD>
hipError_t launch_exposure_as(const ExpoParams& p, uint32_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((pmx_exposure_rows<METHOD>), dim3(blocks), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_exposure(const ExposureArgs& a, void* stream) {
  if (a.n_profiles <= 0 || a.metrics == 0) return hipSuccess;
  ExpoParams p{a.pred, a.P, a.ld_pred, a.prof_off, a.prof_row, a.prof_time, a.n_profiles, (a.P + 63) / 64, 0,
               a.a, a.b, a.threshold, a.metrics, a.out, a.ld_out};
  if (a.n_profiles > (int64_t{1} << 40) / p.n_ctiles) return hipErrorInvalidValue;
  p.n_items = a.n_profiles * p.n_ctiles;
  const int64_t blocks = (p.n_items + 3) / 4;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a.method) {
    case PMX_AUC_LINEAR: return launch_exposure_as<PMX_AUC_LINEAR>(p, static_cast<uint32_t>(blocks), st);
    case PMX_AUC_LIN_UP_LOG_DOWN: return launch_exposure_as<PMX_AUC_LIN_UP_LOG_DOWN>(p, static_cast<uint32_t>(blocks), st);
    case PMX_AUC_LIN_LOG: return launch_exposure_as<PMX_AUC_LIN_LOG>(p, static_cast<uint32_t>(blocks), st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_attainment(const AttainArgs& a, void* stream) {
  if (a.n_profiles <= 0) return hipSuccess;
  const bool wave_owned = a.P <= kAttainWaveMax;
  const int64_t blocks = wave_owned ? (a.n_profiles + 3) / 4 : a.n_profiles;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dispatch(
      [&](auto own, auto post) {
        hipLaunchKernelGGL((pmx_attainment_rows<decltype(own)::value ? 1 : 4, decltype(post)::value>), g, dim3(256), 0, st, a);
        return hipGetLastError();
      },
      wave_owned, a.ll != nullptr);
}

}  // namespace pmx

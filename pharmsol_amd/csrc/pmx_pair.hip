// pmx_pair.hip — the PAIR walker: one (subject, support point) pair per lane.
#include "pmx_lanes.hpp"

namespace pmx {

namespace {

// ------------------------------------------------------------------------------------
// PAIR kernel (analytical): lane = (subject, support point), divergent schedules
// ------------------------------------------------------------------------------------
template <int KID, bool DYN, bool LAG, bool LL>
__global__ __launch_bounds__(kBlock) void pmx_analytical_pair(DevModel m, DevOps ops, const double* __restrict__ theta,
                                                              int64_t P, int64_t S, int32_t batch,
                                                              double* __restrict__ pred, int64_t ld,
                                                              uint8_t* __restrict__ status) {
  using LM = LaneModel<KID>;
  constexpr int NS = LM::NS;
  const int64_t n_pairs = batch ? S : S * P;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool lane_ok = i < n_pairs;
  const int64_t ic = lane_ok ? i : (n_pairs - 1);
  const int64_t s = ops.subj_order[batch ? ic : (ic / P)];
  const int64_t p = batch ? 0 : (ic % P);
  const double* __restrict__ th = theta + (batch ? s : p) * m.nparams;

  LM L;
  lane_setup<KID, DYN>(m, th, L);
  // A lane with complex eigenvalues (lane_setup: all its coefficients are NaN) fails a subject at its first PROP, where
  // the reference's solve panics: the state is NaN from there to the occasion's end, the pair stays failed.  Up to an
  // occasion's first PROP the lane serves the subject like any other.  (The covariate walkers decide per segment.)
  const bool lane_cplx = !DYN && !L.ok;
  uint8_t st_lane0 = PMX_PAIR_OK;
  LagState ls;
  if constexpr (LAG) {
#pragma unroll
    for (int k = 0; k < kMaxLagSlots; ++k) {
      ls.lag[k] = (k < m.n_lag_slots) ? th[m.lag_param[k]] : 0.0;
      ls.cur[k] = ls.end[k] = 0;
      // a negative lag moves the bolus EARLIER, like the reference's `time += l` (structs.rs:629-634); NaN is flagged
      if (k < m.n_lag_slots && ls.lag[k] != ls.lag[k] && st_lane0 == PMX_PAIR_OK) st_lane0 = PMX_PAIR_BAD_LAG;
    }
  }
  const uint8_t st_lane = st_lane0;
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);

  int64_t o = ops.subj_op_off[s];
  const int64_t o1 = lane_ok ? ops.subj_op_off[s + 1] : o;  // idle lanes have an empty stream
  int64_t row = ops.subj_obs_off[s];
  double x[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) x[k] = 0.0;
  double xpad = 0.0;
  double ll_acc = 0.0;
  uint8_t st = st_lane;
  uint8_t st_sticky = PMX_PAIR_OK;  // DYN: first failure of an earlier occasion (see the GRID kernel)
  (void)st_sticky;
  // exec-masked loop: runs while ANY lane of the wave still has ops (each lane exits at its own o1).  Every lane reads
  // its own op, so a fetch is a 64-line gather with nothing to hide its latency behind when the batch is a few
  // thousand pairs (C2: 157 waves on 1024 SIMDs); the ops come as packed 32-byte records (DevOps::op_rec), four
  // at a time: one memory latency per four ops.
  const double4* __restrict__ recs = reinterpret_cast<const double4*>(ops.op_rec);
  for (int64_t og = o; og < o1; og += 4) {
    const int64_t last = o1 - 1;
    double4 q = recs[og];
    double4 q1 = recs[(og + 1 < o1) ? og + 1 : last];
    double4 q2 = recs[(og + 2 < o1) ? og + 2 : last];
    double4 q3 = recs[(og + 3 < o1) ? og + 3 : last];
#pragma unroll 1
    for (int j = 0; j < 4; ++j, q = q1, q1 = q2, q2 = q3) {  // (rotating the records keeps them in registers)
      o = og + j;
      if (o >= o1) break;
      const uint32_t meta = static_cast<uint32_t>(__double_as_longlong(q.x));
      const uint32_t kind = meta & kOpKindMask;
      const int io = static_cast<int>((meta >> kOpIoShift) & kOpIoMask);
      const double a = q.y;
      const double* cov = ops.op_fac + o * (m.n_derived * PMX_MAX_FACTORS);  // this op's covariate factors
      if (kind == OP_PROP) {
        const double r = q.z;
        if constexpr (LAG) {
          lag_prop<LM::ST, NS>(m, ops, ls, q.w, ops.op_t1[o], r, L.coef, th, x);
        } else if constexpr (DYN) {
          if (!lane_advance_dyn<KID>(m, L, cov, x, a, r)) st = PMX_PAIR_COMPLEX_ROOTS;
        } else {
          advance<LM::ST>(L.coef, x, a, r);
        }
        if (lane_cplx) {  // (DYN: never)
          st = PMX_PAIR_COMPLEX_ROOTS;
#pragma unroll
          for (int i = 0; i < NS; ++i) x[i] = nanv;
        }
        xpad = 0.0;
      } else if (kind == OP_OBS) {
        if constexpr (LAG) {  // (see the GRID kernel)
          if (meta >> kOpFlushShift) lag_flush_before<NS>(m, ops, ls, a, th, x);
        }
        double y = lane_out<KID>(m, L, x, xpad, io, cov);
        if ((DYN && st == PMX_PAIR_COMPLEX_ROOTS) || st == PMX_PAIR_BAD_LAG) y = nanv;  // (not DYN: the state is NaN)
        if constexpr (LL) {
          ll_accumulate(ops.ll_obs + row * 4, y, ll_acc);
        } else {
          if (st == PMX_PAIR_OK && !isfinite(y)) st = PMX_PAIR_NONFINITE;
          pred[row * ld + p] = y;
        }
        ++row;
      } else if (kind == OP_BOLUS) {
        const int k = io - m.pm;
        const double amt = a * fa_of(m, th, io);
#pragma unroll
        for (int jj = 0; jj < NS; ++jj) x[jj] += (jj == k) ? amt : 0.0;
        if (m.pm && io == 0) xpad += amt;
      } else {
#pragma unroll
        for (int jj = 0; jj < NS; ++jj) x[jj] = io ? L.xinit[jj] : 0.0;
        xpad = 0.0;
        if constexpr (DYN) {
          if (st_sticky == PMX_PAIR_OK) st_sticky = st;
          st = st_lane;
        }
        if constexpr (LAG) lag_open_occasion<LM::ST, NS>(m, ops, ls, static_cast<int64_t>(a), q.w, L.coef, th, x);
      }
    }
  }
  if constexpr (DYN) {
    if (st_sticky != PMX_PAIR_OK) st = st_sticky;
  }
  if constexpr (LL) {
    if (st == PMX_PAIR_OK && !isfinite(ll_acc)) st = PMX_PAIR_NONFINITE;
    if (lane_ok) ops.ll_out[batch ? s : (s * ops.ll_ld + p)] = (st == PMX_PAIR_OK || st == PMX_PAIR_NONFINITE) ? ll_acc : nanv;
  }
  if (status != nullptr && lane_ok) status[batch ? s : (s * P + p)] = st;  // every pair writes its byte: no memset before the launch
}


template <int KID, bool DYN, bool LAG, bool LL>
hipError_t launch_pair_v(const LaunchArgs& a, const Route& r) {
  hipLaunchKernelGGL((pmx_analytical_pair<KID, DYN, LAG, LL>), dim3(static_cast<uint32_t>(r.blocks)), dim3(r.threads), 0,
                     static_cast<hipStream_t>(a.stream), a.m, a.ops, a.theta, a.P, a.S, a.batch, a.pred, a.ld, a.status);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pair(const LaunchArgs& a, const Route& r) {
  return with_kid(a.m.kernel, [&](auto kid) {
    return dispatch([&](auto dyn, auto lag, auto ll) {  // (lag + covariate-derived constants is rejected at model_create)
      if constexpr (decltype(dyn)::value && decltype(lag)::value) return hipErrorInvalidValue;
      else return launch_pair_v<decltype(kid)::value, decltype(dyn)::value, decltype(lag)::value, decltype(ll)::value>(a, r);
    }, r.dyn && !r.lag, r.lag, r.ll);
  });
}

}  // namespace pmx

// pmx_grid.hip — the generic GRID walker over the op stream (lane mappings: pmx_lanes.hpp).
#include "pmx_lanes.hpp"

namespace pmx {

namespace {

// ------------------------------------------------------------------------------------
// GRID kernel (analytical)
// ------------------------------------------------------------------------------------
template <int KID, bool DYN, bool LAG, bool LL>
// (covariate walkers: 3 waves per SIMD = 168 VGPRs; at 4 the three-compartment rebuild spilled 324 bytes per lane to scratch.
// C5, same box: 4 -> 16.9 ms, 3 -> 16.0 ms, 2 -> 19.8 ms)
#ifndef PMX_DYN_WAVES
#define PMX_DYN_WAVES 3
#endif
__global__ __launch_bounds__(kBlock, (!LAG && LaneModel<KID>::NS <= 2) ? 4 : ((!LAG && DYN) ? PMX_DYN_WAVES : 1)) void pmx_analytical_grid(DevModel m, DevOps ops, const double* __restrict__ theta,
                                                              int64_t P, int64_t S, int32_t s_chunk, int32_t n_ptiles,
                                                              double* __restrict__ pred, int64_t ld,
                                                              uint8_t* __restrict__ status,
                                                              const int32_t* __restrict__ subj_list, int32_t zero_status,
                                                              int32_t prop_slots) {
  using LM = LaneModel<KID>;
  constexpr int NS = LM::NS;
  const int64_t b = blockIdx.x;
  const int32_t ptile = static_cast<int32_t>(b % n_ptiles);
  const int64_t chunk = b / n_ptiles;
  const uint32_t tile = blockDim.x;  // support points per block (64 / 128 / 256: the route's threads)
  const int64_t p = static_cast<int64_t>(ptile) * tile + threadIdx.x;
  const bool lane_ok = p < P;
  const int64_t pc = lane_ok ? p : (P - 1);  // idle lanes shadow the last support point; their stores are masked
  const double* __restrict__ th = theta + pc * m.nparams;
  // DYN: propagators the host marked for reuse wait in LDS, [slot][component][lane] (pmx_compile.cpp, prop cache codes)
  extern __shared__ double prop_cache[];
  constexpr int NPD = static_cast<int>(sizeof(typename LM::S::Prop) / sizeof(double));
  (void)prop_cache;

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
  double ex[LM::S::NE];  // the lane's exponentials of the last PROP (ladder)
#pragma unroll
  for (int i = 0; i < LM::S::NE; ++i) ex[i] = 0.0;

  // the op stream is read-only for the launch and indexed wave-uniformly: constant-address-space pointers
  // turn these into scalar (s_load) fetches
  const auto c_subj_op_off = as_const(ops.subj_op_off);
  const auto c_subj_obs_off = as_const(ops.subj_obs_off);
  const auto c_op_meta = as_const(ops.op_meta);
  const auto c_op_a = as_const(ops.op_a);
  const auto c_op_b = as_const(ops.op_b);
  const auto c_op_t0 = as_const(ops.op_t0);
  const auto c_op_t1 = as_const(ops.op_t1);
  (void)c_op_t0;
  (void)c_op_t1;

  const int64_t s_begin = chunk * s_chunk;
  const int64_t s_end = (s_begin + s_chunk < S) ? (s_begin + s_chunk) : S;
  for (int64_t si = s_begin; si < s_end; ++si) {
    const int64_t s = subj_list ? static_cast<int64_t>(as_const(subj_list)[si]) : si;
    const int64_t o0 = c_subj_op_off[s];
    const int64_t o1 = c_subj_op_off[s + 1];
    int64_t row = c_subj_obs_off[s];
    double x[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = 0.0;
    double xpad = 0.0;
    double ll_acc = 0.0;
    uint8_t st = st_lane;
    uint8_t st_sticky = PMX_PAIR_OK;  // DYN: first failure of an EARLIER occasion (the reference errors out for the whole subject)
    (void)st_sticky;
    // status bytes: no memset precedes the launch.  mode 1 (n_support % 8 == 0, aligned array): the wave clears this
    // subject's 64 bytes with 8 lanes x 8 bytes and only failures are written later; mode 2: every pair's byte is written.
    if (zero_status == 1 && status != nullptr) {
      const uint32_t zl = threadIdx.x & 63u;
      const int64_t zp = static_cast<int64_t>(ptile) * tile + (threadIdx.x & ~63u) + 8 * zl;
      if (zl < 8u && zp < P) *reinterpret_cast<uint64_t*>(status + s * P + zp) = 0ull;
    }
    for (int64_t o = o0; o < o1; ++o) {
      const uint32_t meta = c_op_meta[o];
      const uint32_t kind = meta & kOpKindMask;
      const int io = static_cast<int>((meta >> kOpIoShift) & kOpIoMask);
      const double a = c_op_a[o];
      const double* cov = ops.op_fac + o * (m.n_derived * PMX_MAX_FACTORS);  // this op's covariate factors
      if (kind == OP_PROP) {
        const double r = c_op_b[o];
        if constexpr (LAG) {
          lag_prop<LM::ST, NS>(m, ops, ls, c_op_t0[o], c_op_t1[o], r, L.coef, th, x);
        } else if constexpr (DYN) {
          // bits 24-26: 0 = build; 1 + k = build and keep in slot k; 1 + S + k = take slot k (same length, same
          // covariate factors earlier in this occasion: the same transition matrix).  Wave-uniform: scalar branches.
          const uint32_t rc = (meta >> kOpCacheShift) & kOpCacheMask;
          const uint32_t n_slots = static_cast<uint32_t>(prop_slots);
          typename LM::S::Prop pr;
          if (rc > n_slots) {  // (kept by a segment of the same kind: with a rate -> F and J, without -> F only)
            double tmp[NPD];
#pragma unroll
            for (int k = 0; k < NPD; ++k) tmp[k] = prop_cache[((rc - 1u - n_slots) * NPD + k) * tile + threadIdx.x];
            __builtin_memcpy(&pr, tmp, sizeof(pr));
          } else {
            double q[LM::NKP];
            lane_params_dyn<KID>(m, L, cov, q);
            const bool ok = (r != 0.0) ? make_prop_dyn<LM::ST, true>(q, a, pr) : make_prop_dyn<LM::ST, false>(q, a, pr);
            if (!ok) st = PMX_PAIR_COMPLEX_ROOTS;
            if (rc != 0u) {
              double tmp[NPD];
              __builtin_memcpy(tmp, &pr, sizeof(pr));
#pragma unroll
              for (int k = 0; k < NPD; ++k) prop_cache[((rc - 1u) * NPD + k) * tile + threadIdx.x] = tmp[k];
            }
          }
          if (r != 0.0) LM::S::apply(pr, x, r);
          else LM::S::apply0(pr, x);
        } else {
          // exponential ladder (pmx_plan.cpp ladder_code): bits 27-29 relate this PROP's length to the previous one's
          const uint32_t rung = (meta >> kOpRungShift) & kOpRungMask;
          if (rung == 0u) {
            LM::S::exps(L.coef, a, ex);
          } else if (rung != 1u) {
            ladder_pow<LM::S::NE>(ex, rung);
          }
          step_from_exps<LM::ST>(L.coef, ex, x, r);
        }
        if (lane_cplx) {  // (DYN: never)
          st = PMX_PAIR_COMPLEX_ROOTS;
#pragma unroll
          for (int i = 0; i < NS; ++i) x[i] = nanv;
        }
        xpad = 0.0;  // pm_* wrappers re-pad slot 0 with 0 after every kernel call (analytical/mod.rs:70-75)
      } else if (kind == OP_OBS) {
        if constexpr (LAG) {  // no PROP step in front of this observation: lagged boluses may land before it (bit 31)
          if (meta >> kOpFlushShift) lag_flush_before<NS>(m, ops, ls, a, th, x);
        }
        double y = lane_out<KID>(m, L, x, xpad, io, cov);
        if ((DYN && st == PMX_PAIR_COMPLEX_ROOTS) || st == PMX_PAIR_BAD_LAG) y = nanv;  // (not DYN: the state is NaN)
        if constexpr (LL) {
          ll_accumulate(as_const(ops.ll_obs) + row * 4, y, ll_acc);  // row is wave-uniform: scalar fetches
        } else {
          if (st == PMX_PAIR_OK && !isfinite(y)) st = PMX_PAIR_NONFINITE;
          if (lane_ok) pred[row * ld + p] = y;
        }
        ++row;
      } else if (kind == OP_BOLUS) {
        const int k = io - m.pm;
        const double amt = a * fa_of(m, th, io);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] += (i == k) ? amt : 0.0;
        if (m.pm && io == 0) xpad += amt;
      } else {  // OP_RESET
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = io ? L.xinit[i] : 0.0;
        xpad = 0.0;
        if constexpr (DYN) {  // a new occasion re-derives its coefficients: its rows are finite again, the pair stays failed
          if (st_sticky == PMX_PAIR_OK) st_sticky = st;
          st = st_lane;
        }
        if constexpr (LAG)
          lag_open_occasion<LM::ST, NS>(m, ops, ls, static_cast<int64_t>(a), c_op_t0[o], L.coef, th, x);
      }
    }
    if constexpr (DYN) {
      if (st_sticky != PMX_PAIR_OK) st = st_sticky;
    }
    if constexpr (LL) {
      if (st == PMX_PAIR_OK && !isfinite(ll_acc)) st = PMX_PAIR_NONFINITE;  // NonFiniteLikelihood (prediction.rs:119-124)
      if (lane_ok) ops.ll_out[s * ops.ll_ld + p] = (st == PMX_PAIR_OK || st == PMX_PAIR_NONFINITE) ? ll_acc : nanv;
    }
    if (status != nullptr && lane_ok && (st != PMX_PAIR_OK || zero_status == 2)) {
      if (zero_status == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clearing store above lands first
      status[s * P + p] = st;
    }
  }
}

template <int KID, bool DYN, bool LAG, bool LL>
hipError_t launch_grid_v(const LaunchArgs& a, const Route& r) {
  hipLaunchKernelGGL((pmx_analytical_grid<KID, DYN, LAG, LL>), dim3(static_cast<uint32_t>(r.blocks)), dim3(r.threads), r.lds,
                     static_cast<hipStream_t>(a.stream), a.m, a.ops, a.theta, a.P, r.n, r.s_chunk, r.n_ptiles, a.pred, a.ld, a.status,
                     r.leftover ? a.cls.generic_subjects : nullptr, a.cls.zero_status, a.prop_slots);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_grid(const LaunchArgs& a, const Route& r) {
  return with_kid(a.m.kernel, [&](auto kid) {
    return dispatch([&](auto dyn, auto lag, auto ll) {  // (lag + covariate-derived constants is rejected at model_create)
      if constexpr (decltype(dyn)::value && decltype(lag)::value) return hipErrorInvalidValue;
      else return launch_grid_v<decltype(kid)::value, decltype(dyn)::value, decltype(lag)::value, decltype(ll)::value>(a, r);
    }, r.dyn && !r.lag, r.lag, r.ll);
  });
}

}  // namespace pmx

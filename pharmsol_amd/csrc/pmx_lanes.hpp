// pmx_lanes.hpp — what the analytical kernel units share (internal to libpmx_hip.so; not embedded for hiprtc): the
// lane's model and output helpers, the lag helpers of the generic walkers, the classed kernels' batch size and block
// map.  The kernels themselves, one translation unit per family, each ending in its launch_<family> entry
// (pmx_kernels.hpp):
//   pmx_grid.hip  pmx_dyn3.hip  pmx_steps.hip  pmx_pair.hip      the op-stream walkers
//   pmx_classed.hip  pmx_classed_ll.hip                          the classed kernels
//   pmx_ode_builtin.hip                                          built-in ODE bodies (walkers and steppers: pmx_ode.hpp)
//   pmx_util.hip                                                 log-likelihood tables, status scan, streaming fill
//   pmx_mixture.hip                                              reductions of the log-likelihood matrix: mixture rows, D-function
//   pmx_posterior.hip                                            posterior rows; weighted mean and median of the prediction rows
//   pmx_exposure.hip                                             exposure metrics per (profile, support point); target attainment
//
// One wavefront lane per (subject, support point) pair, two lane mappings:
//
//  GRID  lane = support point (fastest index), a block walks a chunk of subjects.
//        The op stream of a subject is WAVE-UNIFORM: every lane of every wave in the
//        block executes the same BOLUS/OBS/PROP sequence, so op fetches are scalar
//        (s_load through the scalar cache), branches are scalar, and there is no
//        divergence at all.  Stores are pred[row][p0..p0+63]: 512 contiguous bytes per
//        wave-instruction.  Used when n_support >= 32 (NPAG-style grids, C3/C5).
//
//  PAIR  lane = one (subject, support point) pair with its own op cursor; lanes of a
//        wave run different schedules (divergent timelines), the wave loops until every
//        lane's cursor reaches its end (exec-masked loop == ballot of "any lane active").
//        Subjects are pre-sorted by work so neighbouring lanes finish together.
//        Used for n_support < 32 (C2) and for the batch shape (C4: one theta per subject).
//
// States live in registers (1-4 doubles; LDS staging would only add latency), the
// rate-constant-only part of every closed form is hoisted out of the event loop
// (pmx_structures.hpp).  No MFMA: 2-6-state systems have no dense contraction.
//
// Reference contracts: equation/mod.rs:300-358,480-516 (event loop), analytical/mod.rs:299-426,
// ode/mod.rs:609-823 (ODE event loop; diffsol replaced by fixed-step RK4).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include <cmath>
#include <cstdint>

#include "pmx_kernels.hpp"
#include "pmx_structures.hpp"
#include "pmx_device.hpp"

namespace pmx {

namespace {

// derive: derived[d] = ((theta[src] * f0) * f1) (expand/analytical.rs:254,286; bindings.rs:98-117).  The factors
// depend on the op's covariates only, not on the lane: the host evaluated them (pmx_compile.cpp op_fac); `fac` points
// at this op's [n_derived][PMX_MAX_FACTORS] block, `d` = index of the derived value, `base` = theta[src_param].
__device__ __forceinline__ double apply_factors(const DevModel& m, int d, double base, const double* __restrict__ fac) {
  double v = base;
#pragma unroll
  for (int k = 0; k < PMX_MAX_FACTORS; ++k) {
    double f = 1.0;
#pragma unroll
    for (int dd = 0; dd < PMX_MAX_DERIVED; ++dd)
      if (dd == d && k < m.derived[dd].n_factors) f = fac[dd * PMX_MAX_FACTORS + k];
    v = v * f;
  }
  return v;
}

// wide wave-uniform fetches through the scalar unit, placed where they are written (volatile: the compiler neither
// moves nor merges them, and tracks their completion itself)
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
template <class V>
__device__ __forceinline__ V sload_here(const void* p_) {
  const void* p = reinterpret_cast<const void*>(uniform64(reinterpret_cast<int64_t>(p_)));  // (wave-uniform: a scalar address)
  return *(const volatile __attribute__((address_space(4))) V*)(p);
}

// Everything a lane needs besides its state; filled once per lane.
template <int KID>
struct LaneModel {
  static constexpr int ST = kernel_structure(KID);
  using S = Structure<ST>;
  static constexpr int NS = S::NS;
  static constexpr int NKP = kernel_nparams(KID);
  typename S::Coef coef;
  double kp_base[NKP];         // theta[...] for each kernel-order parameter (base value when derived)
  double vol_base[PMX_MAX_OUT];  // theta[...] behind each output's volume (1.0 when none)
  double inv_vol[PMX_MAX_OUT];
  double xinit[NS];
  bool ok;
};

template <int KID, bool DYN>
__device__ __forceinline__ void lane_setup(const DevModel& m, const double* __restrict__ th, LaneModel<KID>& L) {
  using LM = LaneModel<KID>;
#pragma unroll
  for (int j = 0; j < LM::NKP; ++j) {
    int idx = j;
    if (m.n_bind > 0) idx = (m.bind[j].src == PMX_SRC_DERIVED) ? m.derived[m.bind[j].index].src_param : m.bind[j].index;
    L.kp_base[j] = th[idx];
  }
#pragma unroll
  for (int o = 0; o < PMX_MAX_OUT; ++o) {
    double v = 1.0;
    if (o < m.nout) {
      if (m.out[o].vol_src == PMX_SRC_PRIMARY) v = th[m.out[o].vol_index];
      if (m.out[o].vol_src == PMX_SRC_DERIVED) v = th[m.derived[m.out[o].vol_index].src_param];
    }
    L.vol_base[o] = v;
    L.inv_vol[o] = 1.0 / v;
  }
#pragma unroll
  for (int i = 0; i < LM::NS; ++i) {
    const int st = i + m.pm;  // model state index of kernel state i
    L.xinit[i] = (m.has_init && m.init_param[st] >= 0) ? th[m.init_param[st]] : 0.0;
  }
  L.ok = true;
  if constexpr (!DYN) {
    double q[LM::NKP];
    to_native_params<KID>(L.kp_base, q);
    L.ok = LM::S::prepare(q, L.coef);
    // THE rule for a support point with complex eigenvalues, the same on every route of a plain or lagged model: the
    // reference panics inside a solve, and the oracle turns the state into NaN there (pmx_oracle.c, simulate_event).  So
    // such a lane's coefficients are all NaN: whatever a PROP builds from them makes the state NaN, the rows behind it are
    // NaN, and the rows in front of an occasion's first PROP (RESET starts from a finite state) are served like any
    // other lane's.  The pair is PMX_PAIR_COMPLEX_ROOTS once it has propagated.
    if (!L.ok) {
      using Coef = typename LM::S::Coef;  // (doubles and nothing else: pmx_structures.hpp)
      static_assert(std::is_trivially_copyable<Coef>::value && alignof(Coef) == alignof(double) && sizeof(Coef) % sizeof(double) == 0,
                    "a structure's coefficients are a plain block of doubles");
      constexpr int kN = static_cast<int>(sizeof(Coef) / sizeof(double));
      double nans[kN];
#pragma unroll
      for (int i = 0; i < kN; ++i) nans[i] = __longlong_as_double(0x7ff8000000000000LL);
      __builtin_memcpy(&L.coef, nans, sizeof(Coef));
    }
  }
}

// PROP with covariate-derived kernel parameters: this op's rate constants in the structure's native order.
template <int KID>
__device__ __forceinline__ void lane_params_dyn(const DevModel& m, const LaneModel<KID>& L, const double* cov,
                                                double (&q)[LaneModel<KID>::NKP]) {
  using LM = LaneModel<KID>;
  double kp[LM::NKP];
#pragma unroll
  for (int j = 0; j < LM::NKP; ++j) {
    double v = L.kp_base[j];
    if (m.bind[j].src == PMX_SRC_DERIVED) v = apply_factors(m, m.bind[j].index, v, cov);
    kp[j] = v;
  }
  to_native_params<KID>(kp, q);
}
// ... and the segment's propagator applied (fused prepare + make, pmx_structures.hpp make_prop_dyn)
// UNIFORM_R: the rate is wave-uniform (GRID / classed kernels), so a segment without an active infusion can skip the
// response J altogether (a scalar branch); the PAIR kernels' lanes carry their own rates and always build it
template <int KID, bool UNIFORM_R = false>
__device__ __forceinline__ bool lane_advance_dyn(const DevModel& m, const LaneModel<KID>& L, const double* cov,
                                                 double (&x)[LaneModel<KID>::NS], double dt, double r) {
  using LM = LaneModel<KID>;
  double q[LM::NKP];
  lane_params_dyn<KID>(m, L, cov, q);
  typename LM::S::Prop pr;
  bool ok;
  if (UNIFORM_R && r == 0.0) {
    ok = make_prop_dyn<LM::ST, false>(q, dt, pr);
    LM::S::apply0(pr, x);
  } else {
    ok = make_prop_dyn<LM::ST, true>(q, dt, pr);
    LM::S::apply(pr, x, r);
  }
  return ok;
}

template <int KID>
__device__ __forceinline__ double lane_out(const DevModel& m, const LaneModel<KID>& L,
                                           const double (&x)[LaneModel<KID>::NS], double xpad, int outeq,
                                           const double* cov) {
  using LM = LaneModel<KID>;
  // y[o] = x[state] / vol  (e.g. examples/analytical_vs_ode.rs:82-84)
  int state = 0, vsrc = PMX_SRC_NONE, vidx = 0;
  double inv = 1.0, vbase = 1.0;
#pragma unroll
  for (int o = 0; o < PMX_MAX_OUT; ++o) {
    if (o == outeq) {
      state = m.out[o].state;
      vsrc = m.out[o].vol_src;
      vidx = m.out[o].vol_index;
      inv = L.inv_vol[o];
      vbase = L.vol_base[o];
    }
  }
  double xs = select_state<LM::NS>(x, state - m.pm);
  if (m.pm && state == 0) xs = xpad;
  if (vsrc == PMX_SRC_DERIVED) return xs * pmx_rcp(apply_factors(m, vidx, vbase, cov));  // (pmx_structures.hpp: 8 issue slots for 15)
  return xs * inv;
}

// The same for a compile-time output O behind a wave-uniform branch on the op's output index (the lane-valued volume
// terms need no select chain then); no pm_ pad slot.
template <int KID, int O>
__device__ __forceinline__ double lane_out_at(const DevModel& m, const LaneModel<KID>& L, const double (&x)[LaneModel<KID>::NS],
                                              const double* cov) {
  using LM = LaneModel<KID>;
  const double xs = select_state<LM::NS>(x, m.out[O].state);
  if (m.out[O].vol_src == PMX_SRC_DERIVED) return xs * pmx_rcp(apply_factors(m, m.out[O].vol_index, L.vol_base[O], cov));
  return xs * L.inv_vol[O];
}
template <int KID>
__device__ __forceinline__ double lane_out_uniform(const DevModel& m, const LaneModel<KID>& L,
                                                   const double (&x)[LaneModel<KID>::NS], int outeq, const double* cov) {
  static_assert(PMX_MAX_OUT == 4, "one branch per output");
  if (outeq == 0) return lane_out_at<KID, 0>(m, L, x, cov);
  if (outeq == 1) return lane_out_at<KID, 1>(m, L, x, cov);
  if (outeq == 2) return lane_out_at<KID, 2>(m, L, x, cov);
  return lane_out_at<KID, 3>(m, L, x, cov);
}

// (lag / bioavailability helpers shared with the ODE back-end: pmx_device.hpp)

// RESET of a lag model: point the cursors at this occasion's lists and run the boluses that land before the
// occasion's first remaining event (they become the first events of the re-sorted list).
template <int ST, int NS>
__device__ __forceinline__ void lag_open_occasion(const DevModel& m, const DevOps& ops, LagState& ls, int64_t occ,
                                                  double t_first, const typename Structure<ST>::Coef& coef,
                                                  const double* __restrict__ th, double (&x)[NS]) {
#pragma unroll
  for (int k = 0; k < kMaxLagSlots; ++k) {
    if (k < m.n_lag_slots) {
      ls.cur[k] = static_cast<int32_t>(ops.lagb_off[occ * m.n_lag_slots + k]);
      ls.end[k] = static_cast<int32_t>(ops.lagb_off[occ * m.n_lag_slots + k + 1]);
    } else {
      ls.cur[k] = ls.end[k] = 0;
    }
  }
  bool started = false;
  double t = 0.0;
  for (;;) {
    int which;
    const double tau = lag_next(m, ops, ls, which);
    if (!(tau < t_first)) break;
    if (started && tau > t) advance<ST>(coef, x, tau - t, 0.0);
    t = tau;
    started = true;
    lag_apply_bolus<NS>(m, ops, ls, which, th, x);
  }
  if (started && t_first > t && t_first < __longlong_as_double(0x7ff0000000000000LL)) advance<ST>(coef, x, t_first - t, 0.0);
}

// PROP [t0, t1) of a lag model
template <int ST, int NS>
__device__ __forceinline__ void lag_prop(const DevModel& m, const DevOps& ops, LagState& ls, double t0, double t1, double r,
                                         const typename Structure<ST>::Coef& coef, const double* __restrict__ th,
                                         double (&x)[NS]) {
  double t = t0;
  for (;;) {
    int which;
    const double tau = lag_next(m, ops, ls, which);
    if (!(tau < t1)) break;
    if (tau > t) {
      advance<ST>(coef, x, tau - t, r);
      t = tau;
    }
    lag_apply_bolus<NS>(m, ops, ls, which, th, x);
  }
  if (t1 > t) advance<ST>(coef, x, t1 - t, r);
}

// ------------------------------------------------------------------------------------
// classed kernels: G subjects of one class per lane
// ------------------------------------------------------------------------------------
template <int KID>
struct ClassBatch {
  static constexpr int G = (LaneModel<KID>::NS <= 2) ? 8 : 4;
};

// XCD-aware block -> tile map.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8
// share an XCD and its L2).  The n_ptiles column tiles of one chunk-block together write whole
// prediction rows; placing them on ONE XCD lets that L2 assemble full rows / whole per-subject
// regions before write-back instead of scattering 2 KB pieces of every row over n_ptiles L2s.
// (speed only: any placement is correct)
// chunk-blocks take chunks cblock, cblock + n_cblocks, ... (grid stride): the blocks resident at one moment then
// work on neighbouring chunks, which keeps each of the G write fronts compact (see build_class_plan `spread`)
struct ClassedBlock {
  int32_t ptile;
  int64_t cblock, n_cblocks;
};
__device__ __forceinline__ ClassedBlock classed_block(int32_t n_ptiles) {
  const int64_t b = blockIdx.x;
  const int64_t group = b / (8 * n_ptiles);
  const int32_t local = static_cast<int32_t>(b % (8 * n_ptiles));
  return {local / 8, group * 8 + (local % 8), static_cast<int64_t>(gridDim.x) / n_ptiles};
}

}  // namespace

}  // namespace pmx

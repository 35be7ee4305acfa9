// pmx_ode_builtin.hip — the built-in diffeq bodies on the ODE walkers of pmx_ode.hpp.
#include <hip/hip_runtime.h>

#include <type_traits>

#include <cmath>
#include <cstdint>

#include "pmx_kernels.hpp"
#include "pmx_structures.hpp"
#include "pmx_device.hpp"
#include "pmx_ode.hpp"

namespace pmx {
namespace {

// ------------------------------------------------------------------------------------
// ODE: built-in diffeq bodies (the walkers and the RK4 stepper are in pmx_ode.hpp)
// ------------------------------------------------------------------------------------
template <int MODEL>
struct OdeModel;

template <>
struct OdeModel<PMX_ODE_ONE_CMT_IV> {  // examples/ode_readme.rs:17-19
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 1, NP = 1, CENTRAL = 0;
  static constexpr int NR = 1;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -p[0] * x[0];
  }
};
template <>
struct OdeModel<PMX_ODE_ONE_CMT_ORAL> {
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 2, NP = 2, CENTRAL = 1;
  static constexpr int NR = 2;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -p[0] * x[0];
    dx[1] = p[0] * x[0] - p[1] * x[1];
  }
};
template <>
struct OdeModel<PMX_ODE_TWO_CMT_IV> {  // two_compartment_models.rs:131-136
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 2, NP = 3, CENTRAL = 0;
  static constexpr int NR = 2;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -p[0] * x[0] - p[1] * x[0] + p[2] * x[1];
    dx[1] = p[1] * x[0] - p[2] * x[1];
  }
};
template <>
struct OdeModel<PMX_ODE_TWO_CMT_ORAL> {  // two_compartment_models.rs:188-194, p=[ke,ka,kcp,kpc]
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 3, NP = 4, CENTRAL = 1;
  static constexpr int NR = 3;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -p[1] * x[0];
    dx[1] = -p[0] * x[1] + p[1] * x[0] - p[2] * x[1] + p[3] * x[2];
    dx[2] = p[2] * x[1] - p[3] * x[2];
  }
};
template <>
struct OdeModel<PMX_ODE_THREE_CMT_IV> {
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 3, NP = 5, CENTRAL = 0;
  static constexpr int NR = 3;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -(p[0] + p[1] + p[2]) * x[0] + p[3] * x[1] + p[4] * x[2];
    dx[1] = p[1] * x[0] - p[3] * x[1];
    dx[2] = p[2] * x[0] - p[4] * x[2];
  }
};
template <>
struct OdeModel<PMX_ODE_THREE_CMT_ORAL> {
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 4, NP = 6, CENTRAL = 1;
  static constexpr int NR = 4;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    dx[0] = -p[0] * x[0];
    dx[1] = p[0] * x[0] - (p[1] + p[2] + p[3]) * x[1] + p[4] * x[2] + p[5] * x[3];
    dx[2] = p[2] * x[1] - p[4] * x[2];
    dx[3] = p[3] * x[1] - p[5] * x[3];
  }
};
template <>
struct OdeModel<PMX_ODE_ONE_CMT_MM> {  // p=[vmax,km,v]
  static constexpr bool CUSTOM = false;
  static constexpr int NS = 1, NP = 3, CENTRAL = 0;
  static constexpr int NR = 1;
  __device__ __forceinline__ static void rhs(const double* p, const double (&x)[NS], double (&dx)[NS]) {
    const double cc = x[0] / p[2];
    dx[0] = -p[0] * cc / (p[1] + cc);
  }
};


template <int MODEL, bool LAG, bool LL, int SOLV>
__global__ __launch_bounds__(kBlock) void pmx_ode_rk4_grid(DevModel m, DevOps ops, const double* __restrict__ theta,
                                                           int64_t P, int64_t S, int32_t s_chunk, int32_t n_ptiles,
                                                           double* __restrict__ pred, int64_t ld,
                                                           uint8_t* __restrict__ status) {
  ode_grid_body<OdeModel<MODEL>, LAG, LL, SOLV>(m, ops, theta, P, S, s_chunk, n_ptiles, pred, ld, status);
}

template <int MODEL, bool LAG, bool LL, int SOLV>
__global__ __launch_bounds__(kBlock) void pmx_ode_rk4_pair(DevModel m, DevOps ops, const double* __restrict__ theta,
                                                           int64_t P, int64_t S, int32_t batch,
                                                           double* __restrict__ pred, int64_t ld,
                                                           uint8_t* __restrict__ status) {
  ode_pair_body<OdeModel<MODEL>, LAG, LL, SOLV>(m, ops, theta, P, S, batch, pred, ld, status);
}


template <int MODEL>
hipError_t launch_ode_m(const LaunchArgs& a, const Route& r) {
  // (lag, ll, the stepper counted down, pair: the order this unit has always instantiated its kernels in, so its assembly
  // compares file against file.  The same instantiation serves both adaptive steppers: DevModel::ode_stiff)
  return dispatch([&](auto lag, auto ll) {
    return with_solv(kSolvers[r.solver].solv, [&](auto solv) {
      return dispatch([&](auto pair) {
        constexpr bool LAG = decltype(lag)::value, LL = decltype(ll)::value;
        constexpr int SOLV = decltype(solv)::value;
        hipStream_t st = static_cast<hipStream_t>(a.stream);
        const dim3 grid(static_cast<uint32_t>(r.blocks)), block(r.threads);
        if constexpr (!decltype(pair)::value)
          hipLaunchKernelGGL((pmx_ode_rk4_grid<MODEL, LAG, LL, SOLV>), grid, block, 0, st, a.m, a.ops, a.theta, a.P, a.S,
                             r.s_chunk, r.n_ptiles, a.pred, a.ld, a.status);
        else
          hipLaunchKernelGGL((pmx_ode_rk4_pair<MODEL, LAG, LL, SOLV>), grid, block, 0, st, a.m, a.ops, a.theta, a.P, a.S,
                             a.batch, a.pred, a.ld, a.status);
        return hipGetLastError();
      }, r.mode != MODE_GRID);
    });
  }, r.lag, r.ll);
}

}  // namespace

hipError_t launch_ode(const LaunchArgs& a, const Route& r) {
  switch (a.m.kernel) {
    case PMX_ODE_ONE_CMT_IV: return launch_ode_m<PMX_ODE_ONE_CMT_IV>(a, r);
    case PMX_ODE_ONE_CMT_ORAL: return launch_ode_m<PMX_ODE_ONE_CMT_ORAL>(a, r);
    case PMX_ODE_TWO_CMT_IV: return launch_ode_m<PMX_ODE_TWO_CMT_IV>(a, r);
    case PMX_ODE_TWO_CMT_ORAL: return launch_ode_m<PMX_ODE_TWO_CMT_ORAL>(a, r);
    case PMX_ODE_THREE_CMT_IV: return launch_ode_m<PMX_ODE_THREE_CMT_IV>(a, r);
    case PMX_ODE_THREE_CMT_ORAL: return launch_ode_m<PMX_ODE_THREE_CMT_ORAL>(a, r);
    case PMX_ODE_ONE_CMT_MM: return launch_ode_m<PMX_ODE_ONE_CMT_MM>(a, r);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pmx

// pmx_solvers.hpp — THE solver table of the host: one row per PMX_SOLVER_* value the library accepts, with everything
// the host knows about that solver.  The model checks (pmx_api.cpp), key_for / finish_model / plan_routes / route_name
// (pmx_launch.cpp), the generated translation units (pmx_jit_source.cpp) and launch_ode (pmx_ode_builtin.hip) all read it.
#pragma once

#include <cstdint>

#include "pmx_devtypes.hpp"

namespace pmx {

struct SolverRow {
  int32_t id;        // PMX_SOLVER_*
  int32_t solv;      // the walkers' compile-time stepper (SOLV_*, pmx_devtypes.hpp)
  bool stiff;        // the adaptive step is ROS2 (DevModel::ode_stiff)
  bool needs_tol;    // ode_rtol > 0 and ode_atol > 0 are required
  bool want_times;   // the stream carries absolute piece times: the stepper walks [t0, t1] itself
  const char* name;  // fragment of the kernel names (route_name)
};
inline constexpr SolverRow kSolvers[] = {
    {PMX_SOLVER_RK4, SOLV_RK4, false, false, false, "rk4"},
    {PMX_SOLVER_DOPRI5, SOLV_ADAPT, false, true, true, "dopri5"},
    {PMX_SOLVER_ROS2, SOLV_ADAPT, true, true, true, "ros2"},
    {PMX_SOLVER_RK4_CHECKED, SOLV_CHECKED, false, true, false, "rk4_checked"},  // (walks the fixed-step stream as it is)
    {PMX_SOLVER_AUTO, SOLV_AUTO, false, true, true, "auto"}};                   // (its stream is dopri5's)
constexpr int kNumSolvers = static_cast<int>(sizeof(kSolvers) / sizeof(kSolvers[0]));

// the row of a descriptor's ode_solver; null for 4 (no solver) and every other unknown value
inline const SolverRow* solver_row(int32_t ode_solver) {
  for (const SolverRow& r : kSolvers)
    if (r.id == ode_solver) return &r;
  return nullptr;
}

// The SOLV_* variants [begin, end) the translation unit of a run-time-compiled ODE model of that solver holds (fixed at
// creation): the fixed-step and the adaptive walkers together, as ever, or the one walker of a later solver INSTEAD.
struct SolvRange { int begin, end; };
inline SolvRange jit_solv_range(int32_t ode_solver) {
  const int v = solver_row(ode_solver)->solv;
  return v <= SOLV_ADAPT ? SolvRange{SOLV_RK4, SOLV_ADAPT + 1} : SolvRange{v, v + 1};
}

}  // namespace pmx

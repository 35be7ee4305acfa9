// pmx_jit_source.hpp — what a run-time-compiled model is compiled from (JitSpec) and the text generated for it.
// Pure host code: no HIP header (pmx_jit.hpp holds the hiprtc compile and the module load).
#pragma once

#include <cstdint>
#include <string>

#include "../../include/pmx.h"
#include "pmx_devtypes.hpp"
#include "pmx_solvers.hpp"

namespace pmx {

enum JitKind { JIT_ODE = 0, JIT_ANALYTICAL = 1, JIT_ODE_USER = 2 };

struct JitSpec {
  JitKind kind = JIT_ODE;
  // The model.  JIT_ODE, a diffeq body on the state-machine kernels (pmx_ode.hpp), reads its sizes; the closure walkers -
  // JIT_ANALYTICAL (pmx_analytical.hpp), and JIT_ODE_USER (pmx_ode_user.hpp), an ODE model whose lag / fa / derive are
  // closures too or whose dynamics takes the bolus vector - also what the generator turns into code for every closure
  // `source` leaves out.
  pmx_model_desc desc{};
  std::string source;     // the user's definitions (pmx_dynamics, pmx_outputs, ...: include/pmx.h)
  uint32_t fns = 0;       // closure walkers: the closures `source` defines (PMX_FN_*)
  bool has_init = false;  // JIT_ODE: `source` defines pmx_init
  // ODE models: the descriptor's ode_solver (a PMX_SOLVER_* value); decides which walkers the translation unit holds
  // (jit_solv_range, pmx_solvers.hpp)
  int32_t solver = PMX_SOLVER_RK4;
  bool big_lists = false;  // closure walkers: compile the > 64-boluses-per-occasion path in (PMX_USER_BIG_LISTS, pmx_userlag.hpp)
};

// THE entry points of a translation unit, one row per JitKind: pmx_jit_<stem>_<lag><ll><solv> instantiates `body` with
// <UserModel, lag, ll, SOLV_*>.  A dimension the kind does not have contributes no digit and no template argument, and is
// index 0 of JitModule::fn.  The wrapper emitter (pmx_jit_source.cpp) and jit_load (pmx_jit.cpp) read it.
struct JitEntryRow {
  const char* stem[2];  // [mode: 0 GRID, 1 PAIR]
  const char* body[2];  // the walker's body template (pmx_ode.hpp, pmx_analytical.hpp, pmx_ode_user.hpp)
  bool lag;             // lag x no lag variants
  bool solver;          // one variant per SOLV_* of jit_solv_range(spec.solver)
};
inline constexpr JitEntryRow kJitEntries[3] = {{{"grid", "pair"}, {"ode_grid_body", "ode_pair_body"}, true, true},
                                               {{"agrid", "apair"}, {"user_grid_body", "user_pair_body"}, false, false},
                                               {{"ugrid", "upair"}, {"uode_grid_body", "uode_pair_body"}, false, true}};
std::string jit_entry_name(const JitEntryRow& row, int mode, int lag, int ll, int solv);
// the solver variants the translation unit of `s` holds: one index, 0, for a kind without the dimension
inline SolvRange jit_entry_solvers(const JitSpec& s) { return kJitEntries[s.kind].solver ? jit_solv_range(s.solver) : SolvRange{0, 1}; }

// The translation unit handed to hiprtc (user source + policy + the kernel wrappers: 16 for an ODE model - GRID/PAIR x
// lag x log-likelihood x solver -, 4 for an analytical one - GRID/PAIR x log-likelihood -, 8 for an ODE model with
// user lag / fa closures - GRID/PAIR x log-likelihood x solver).  "solver" = the SOLV_* variants of jit_solv_range(spec.solver):
// two for a fixed-step or adaptive model, one (8 and 4 wrappers) for a checked-RK4 or an auto model.
std::string jit_translation_unit(const JitSpec& spec);

// Source text (pmx_derive) of an ANALYTICAL descriptor's derived values (desc.derived[]: theta * covariate factors), for
// descriptor models the library's own kernels do not take (lag time together with covariate-derived rate constants or
// pm_* indexing, more than four lagged inputs): such a model runs on the user-closure walker, every other closure
// generated from the descriptor as usual.
std::string analytical_descriptor_source(const pmx_model_desc& d);

// Source text (pmx_dynamics / pmx_outputs / pmx_init) of a BUILT-IN diffeq body whose parameters / volumes are derived
// from covariates through the descriptor (desc.derived[], desc.bind[]): the covariates are bound at the stage time.
std::string ode_descriptor_source(const pmx_model_desc& d);

}  // namespace pmx

// pmx_model.cpp — model creation: pmx_model_create, pmx_model_create_custom, pmx_model_create_user and the two
// pmx_debug_jit_source* views of what they compile.
//
// A (descriptor, closure set) pair takes one of five creation paths (kPaths).  The path's row says what of the descriptor
// is checked, allowed or forbidden; check_desc applies the row, each check written once; resolve picks the path and
// returns everything that fixes the model - also when one path hands the model to another (DESIGN.md "Model creation").
#include <cstdlib>
#include <cstring>

#include "pmx_internal.hpp"
#include "pmx_structures.hpp"  // kernel_nparams()

namespace {

// which table the state and parameter counts of a path's structure come from
enum Structure {
  S_ANALYTICAL,  // d->kernel names a built-in structure (or PMX_K_CUSTOM on the user path: the source's pmx_eq)
  S_ODE_BODY,    // d->kernel names a built-in diffeq body
  S_SOURCE       // kernel = PMX_ODE_CUSTOM: the source text is the structure
};
enum Outputs { OUT_CHECKED, OUT_UNLESS_CLOSURE, OUT_UNCHECKED };

constexpr const char* kNdrugs = "ndrugs out of range";
constexpr const char* kNdrugsUser = "ndrugs out of range (1..8 for a model with user closures)";
constexpr const char* kNoPmOde =
    "pm_* indexing is a wrapper of the analytical structures (analytical/mod.rs:62-90): it does not apply to ODE models";
constexpr const char* kNoDescCustom =
    "derived-parameter descriptors / pm indexing do not apply to custom ODE bodies (compute them in the body)";
constexpr const char* kNeedCustom = "custom models need eq_kind = PMX_EQ_ODE and kernel = PMX_ODE_CUSTOM";
constexpr const char* kNeedCustomUser = "ODE models with user closures need kernel = PMX_ODE_CUSTOM";
constexpr const char* kNoBindUserOde = "bind[] / pm indexing do not apply to ODE models with user closures";

// One row per creation path.  A null no_* text: the field is allowed.  The rows differ in more places than the paths
// need; every difference is as found (DESIGN.md lists them), none is decided here.
struct PathRow {
  Structure structure;
  const char* wrong_kernel;  // S_SOURCE: the refusal of any other (eq_kind, kernel)
  int ndrugs_min;
  const char* ndrugs_text;
  int nparams_min;
  int n_derived_max;
  bool derived_desc;                          // derived[] is read, so its entries are checked
  const char *no_derived, *no_bind, *no_pm;   // refusal of n_derived != 0 / n_bind != 0 / pmetrics_indexing
  bool numerics;                              // check_ode_numerics
  bool bolus_dest, infusion_dest, init_param;
  Outputs out;
};
// built-in analytical structure, built-in diffeq body, custom diffeq body (state-machine kernels), user analytical, user ODE (general walker)
enum PathId { P_ANALYTICAL, P_ODE_BODY, P_CUSTOM, P_USER_ANALYTICAL, P_USER_ODE };
// clang-format off
const PathRow kPaths[] = {
  //                     structure     wrong_kernel     nd>= text      np>= n_derived<=           derived[] no_derived     no_bind         no_pm           numerics bolus infus  init   out[]
  /*P_ANALYTICAL*/      {S_ANALYTICAL, nullptr,         0, kNdrugs,     0, PMX_MAX_DERIVED,      true,     nullptr,       nullptr,        nullptr,        false,   false, false, true,  OUT_CHECKED},
  /*P_ODE_BODY*/        {S_ODE_BODY,   nullptr,         0, kNdrugs,     0, PMX_MAX_DERIVED,      true,     nullptr,       nullptr,        kNoPmOde,       true,    true,  true,  true,  OUT_CHECKED},
  /*P_CUSTOM*/          {S_SOURCE,     kNeedCustom,     0, kNdrugs,     1, 0,                    false,    kNoDescCustom, kNoDescCustom,  kNoDescCustom,  true,    true,  false, false, OUT_UNCHECKED},
  /*P_USER_ANALYTICAL*/ {S_ANALYTICAL, nullptr,         1, kNdrugsUser, 1, PMX_MAX_USER_DERIVED, false,    nullptr,       nullptr,        nullptr,        false,   false, false, true,  OUT_UNLESS_CLOSURE},
  /*P_USER_ODE*/        {S_SOURCE,     kNeedCustomUser, 1, kNdrugsUser, 1, PMX_MAX_USER_DERIVED, false,    nullptr,       kNoBindUserOde, kNoBindUserOde, true,    true,  false, true,  OUT_UNCHECKED},
};
// clang-format on

int32_t bad(const char* msg) { return fail(PMX_ERR_INVALID_ARGUMENT, msg); }

// ---- the checks, each written once ----------------------------------------------------------------------------------
int32_t check_sizes(const pmx_model_desc* d, const PathRow& row) {
  if (d->nstates < 1 || d->nstates > PMX_MAX_STATES) return bad("nstates out of range");
  if (d->ndrugs < row.ndrugs_min || d->ndrugs > PMX_MAX_INPUTS) return bad(row.ndrugs_text);
  if (d->nout < 1 || d->nout > PMX_MAX_OUT) return bad("nout out of range");
  if (d->nparams < row.nparams_min || d->nparams > PMX_MAX_PARAMS) return bad("nparams out of range");
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES) return bad("n_covariates out of range");
  if (row.no_derived && d->n_derived != 0) return bad(row.no_derived);
  if (d->n_derived < 0 || d->n_derived > row.n_derived_max) return bad("n_derived out of range");
  if (row.no_bind && d->n_bind != 0) return bad(row.no_bind);
  if (row.no_pm && d->pmetrics_indexing) return bad(row.no_pm);
  return PMX_OK;
}

int32_t check_derived(const pmx_model_desc* d) {
  for (int i = 0; i < d->n_derived; ++i) {
    const pmx_derived& dd = d->derived[i];
    if (dd.src_param < 0 || dd.src_param >= d->nparams) return bad("derived.src_param out of range");
    if (dd.n_factors < 0 || dd.n_factors > PMX_MAX_FACTORS) return bad("derived.n_factors out of range");
    for (int k = 0; k < dd.n_factors; ++k)
      if (dd.f[k].op != PMX_F_NONE && (dd.f[k].cov < 0 || dd.f[k].cov >= d->n_covariates))
        return bad("derived factor covariate out of range");
  }
  return PMX_OK;
}

// states / parameters of the built-in structures (AnalyticalKernel::state_count analysis.rs:259-270; kernel_nparams) and diffeq bodies
const int kAnalyticalStates[PMX_K_ANALYTICAL_COUNT] = {1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4};
const struct { int nstates, nparams; } kOdeBody[PMX_ODE_MODEL_COUNT] = {{1, 1}, {2, 2}, {2, 3}, {3, 4}, {3, 5}, {4, 6}, {1, 3}};

int32_t check_bind(const pmx_model_desc* d) {
  for (int j = 0; j < d->n_bind; ++j) {
    const pmx_bind& b = d->bind[j];
    if (b.src == PMX_SRC_PRIMARY) {
      if (b.index < 0 || b.index >= d->nparams) return bad("bind index out of range");
    } else if (b.src == PMX_SRC_DERIVED) {
      if (b.index < 0 || b.index >= d->n_derived) return bad("bind derived index out of range");
    } else
      return bad("bind.src must be PRIMARY or DERIVED");
  }
  return PMX_OK;
}

// the structure has the states and parameters the descriptor gives it; bind[], where the structure reads it
int32_t check_structure(const pmx_model_desc* d, const PathRow& row) {
  switch (row.structure) {
    case S_SOURCE:
      if (d->eq_kind != PMX_EQ_ODE || d->kernel != PMX_ODE_CUSTOM) return bad(row.wrong_kernel);
      return PMX_OK;
    case S_ANALYTICAL: {
      if (d->kernel == PMX_K_CUSTOM) return PMX_OK;  // (user path only, check_closures: the source's pmx_eq, which reads no bind[])
      if (d->kernel < 0 || d->kernel >= PMX_K_ANALYTICAL_COUNT) return bad("unknown analytical kernel");
      if (d->nstates < kAnalyticalStates[d->kernel] + (d->pmetrics_indexing ? 1 : 0)) return bad("model has fewer states than its structure");
      const int np = pmx::kernel_nparams(d->kernel);
      if (d->n_bind == 0 && d->nparams < np) return bad("too few parameters for the structure");
      if (d->n_bind != 0 && d->n_bind != np) return bad("n_bind must equal the structure's parameter count");
      return check_bind(d);
    }
    case S_ODE_BODY:
      if (d->kernel < 0 || d->kernel >= PMX_ODE_MODEL_COUNT) return bad("unknown ODE model");
      if (d->nstates < kOdeBody[d->kernel].nstates) return bad("model has fewer states than its diffeq");
      if (d->nparams < kOdeBody[d->kernel].nparams) return bad("too few parameters for the diffeq");
      if (d->n_bind != 0 && d->n_bind != kOdeBody[d->kernel].nparams) return bad("n_bind must equal the diffeq's parameter count");
      return check_bind(d);
  }
  return PMX_OK;
}

// the numeric part of an ODE descriptor: step ceiling, solver, its tolerances
int32_t check_ode_numerics(const pmx_model_desc* d) {
  if (!(d->rk4_h_max > 0.0)) return bad("rk4_h_max must be > 0");
  const pmx::SolverRow* solver = pmx::solver_row(d->ode_solver);
  if (!solver) return bad("unknown ode_solver");
  if (solver->needs_tol && !(d->ode_rtol > 0.0 && d->ode_atol > 0.0))
    return bad("the adaptive solvers and checked RK4 need ode_rtol > 0 and ode_atol > 0");
  return PMX_OK;
}

int32_t check_routes(const pmx_model_desc* d, const PathRow& row) {
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
    if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams) return bad("lag_param / fa_param out of range");
    if ((row.bolus_dest && d->bolus_dest[i] >= d->nstates) || (row.infusion_dest && d->infusion_dest[i] >= d->nstates))
      return bad("route destination out of range");
  }
  return PMX_OK;
}

int32_t check_outputs(const pmx_model_desc* d) {
  for (int o = 0; o < d->nout; ++o) {
    const pmx_out& oo = d->out[o];
    if (oo.state < 0 || oo.state >= d->nstates) return bad("out.state out of range");
    if (oo.vol_src == PMX_SRC_PRIMARY && (oo.vol_index < 0 || oo.vol_index >= d->nparams)) return bad("out.vol_index out of range");
    if (oo.vol_src == PMX_SRC_DERIVED && (oo.vol_index < 0 || oo.vol_index >= d->n_derived))
      return bad("out.vol_index (derived) out of range");
  }
  return PMX_OK;
}

int32_t check_init(const pmx_model_desc* d) {
  for (int i = 0; i < PMX_MAX_STATES; ++i)
    if (d->init_param[i] >= d->nparams) return bad("init_param out of range");
  return PMX_OK;
}

// which closures the source of a user model must, may and may not define (pmx.h "user closures for either back-end")
int32_t check_closures(const pmx_model_desc* d, PathId path, uint32_t fns) {
  if (path != P_USER_ANALYTICAL && path != P_USER_ODE) return PMX_OK;
  if (d->n_derived > 0 && !(fns & PMX_FN_DERIVE)) return bad("n_derived > 0 needs PMX_FN_DERIVE (desc.derived[] is not read for user models)");
  if (path == P_USER_ODE) {
    const bool dyn = (fns & PMX_FN_DYNAMICS) != 0, dynb = (fns & PMX_FN_DYNAMICS_BOLUS) != 0;
    if (dyn == dynb) return bad("ODE models define pmx_dynamics OR pmx_dynamics_bolus (PMX_FN_DYNAMICS | PMX_FN_DYNAMICS_BOLUS)");
    if (!(fns & PMX_FN_OUTPUTS)) return bad("ODE models define pmx_outputs (PMX_FN_OUTPUTS)");
    if (fns & (PMX_FN_SEQ_EQ | PMX_FN_EQ)) return bad("PMX_FN_SEQ_EQ / PMX_FN_EQ belong to analytical models");
    return PMX_OK;
  }
  if (fns & PMX_FN_DYNAMICS) return bad("PMX_FN_DYNAMICS belongs to ODE models");
  if (d->kernel == PMX_K_CUSTOM) {
    if (d->pmetrics_indexing) return bad("pm_* indexing wraps a built-in structure: it does not apply to a user propagator (pmx_eq)");
    if (!(fns & PMX_FN_EQ)) return bad("kernel = PMX_K_CUSTOM needs PMX_FN_EQ");
  } else if (fns & PMX_FN_EQ)
    return bad("PMX_FN_EQ needs kernel = PMX_K_CUSTOM");
  return PMX_OK;
}

int32_t check_desc(const pmx_model_desc* d, PathId path, uint32_t fns) {
  const PathRow& row = kPaths[path];
  int32_t rc = check_closures(d, path, fns);
  if (rc == PMX_OK) rc = check_sizes(d, row);
  if (rc == PMX_OK && row.derived_desc) rc = check_derived(d);
  if (rc == PMX_OK) rc = check_structure(d, row);
  if (rc == PMX_OK && row.numerics) rc = check_ode_numerics(d);
  if (rc == PMX_OK) rc = check_routes(d, row);
  if (rc == PMX_OK && (row.out == OUT_CHECKED || (row.out == OUT_UNLESS_CLOSURE && !(fns & PMX_FN_OUTPUTS)))) rc = check_outputs(d);
  if (rc == PMX_OK && row.init_param) rc = check_init(d);
  return rc;
}

// ---- what of a valid descriptor decides its walker ------------------------------------------------------------------
int count_lagged(const pmx_model_desc& d) {
  int n = 0;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) n += d.lag_param[i] >= 0;
  return n;
}
bool binds_covariate_factors(const pmx_model_desc& d) {  // a rate constant bound to a derived value that varies with a covariate
  for (int j = 0; j < d.n_bind; ++j)
    if (d.bind[j].src == PMX_SRC_DERIVED && d.derived[d.bind[j].index].n_factors > 0) return true;
  return false;
}
bool inits_from_params(const pmx_model_desc& d) {
  for (int i = 0; i < d.nstates && i < PMX_MAX_STATES; ++i)
    if (d.init_param[i] >= 0) return true;
  return false;
}

// Everything that fixes a model: the path that takes it and the model itself, complete but for its code object - the
// descriptor as stored, pmx_model's flags (key_for and finish_model read them), jit_spec - and what a compile failure says.
struct Resolved {
  PathId path = P_ANALYTICAL;
  std::unique_ptr<pmx_model> m = std::make_unique<pmx_model>();
  bool compiled = false;                         // m->jit_spec is filled: the model carries a hiprtc code object
  int32_t fail_code = PMX_ERR_INVALID_ARGUMENT;  // a compile failure: the caller's text is at fault, or ours (PMX_ERR_HIP)
  const char* fail_what = "model source";
  void generated(const char* what) { fail_code = PMX_ERR_HIP, fail_what = what; }
};

int32_t spec_solver(const pmx_model_desc& d) { return d.eq_kind == PMX_EQ_ODE ? d.ode_solver : PMX_SOLVER_RK4; }  // (JitSpec::solver)

// what every run-time-compiled model is compiled from
void take_source(Resolved* r, pmx::JitKind kind, std::string source, uint32_t fns) {
  pmx_model* m = r->m.get();
  m->custom = true;
  pmx::JitSpec& sp = m->jit_spec;
  sp.kind = kind;
  sp.desc = m->d;
  sp.source = std::move(source);
  sp.fns = fns;
  sp.has_init = m->has_init;
  sp.solver = spec_solver(m->d);
  r->compiled = true;
}

// a diffeq body on the state-machine kernels (pmx_ode.hpp): theta-indexed lag / fa, at most kMaxLagSlots lagged inputs
void take_state_machine_body(Resolved* r, std::string source, bool has_init) {
  r->m->has_init = has_init;
  take_source(r, pmx::JIT_ODE, std::move(source), 0);
}

// The closure walkers (pmx_analytical.hpp; pmx_ode_user.hpp, the general ODE walker, which sorts any number of lagged
// boluses): every closure the source leaves out is generated from the descriptor.
void take_closure_walker(Resolved* r, std::string source, uint32_t fns, bool descriptor_walker = false) {
  pmx_model* m = r->m.get();
  m->dyn = false;
  m->user_fns = fns;
  m->user_ode = m->d.eq_kind == PMX_EQ_ODE;
  m->user_lag = descriptor_walker || (fns & PMX_FN_ROUTE_LAG) != 0 || count_lagged(m->d) > 0;
  m->has_init = true;  // (RESET ops always carry the occasion-index flag; the policy's init may be empty)
  take_source(r, m->user_ode ? pmx::JIT_ODE_USER : pmx::JIT_ANALYTICAL, std::move(source), fns);
}

// A diffeq body with more than kMaxLagSlots lagged inputs leaves its path (the state-machine kernels keep four lag
// cursors) for the general walker.  The user-ODE row applies to it as to any model on that walker.
int32_t hand_to_general_ode_walker(Resolved* r, std::string source, uint32_t fns) {
  r->path = P_USER_ODE;
  const int32_t rc = check_desc(&r->m->d, P_USER_ODE, fns);
  if (rc == PMX_OK) take_closure_walker(r, std::move(source), fns);
  return rc;
}

enum Entry { ENTRY_CREATE, ENTRY_CUSTOM, ENTRY_USER };

int32_t resolve(Entry entry, const pmx_model_desc* d, const char* source, uint32_t fns, int32_t has_init, Resolved* r) {
  if (!d || (entry != ENTRY_CREATE && !source)) return bad("null argument");
  if (entry == ENTRY_USER && d->eq_kind == PMX_EQ_ODE && d->n_derived == 0 &&
      (fns & ~static_cast<uint32_t>(PMX_FN_INIT)) == (PMX_FN_DYNAMICS | PMX_FN_OUTPUTS)) {
    entry = ENTRY_CUSTOM;  // no closure beyond the body: theta-indexed lag / fa, the state-machine kernels
    has_init = (fns & PMX_FN_INIT) ? 1 : 0;
  }
  if (entry == ENTRY_CUSTOM)
    r->path = P_CUSTOM;
  else if (d->eq_kind == PMX_EQ_ANALYTICAL)
    r->path = entry == ENTRY_USER ? P_USER_ANALYTICAL : P_ANALYTICAL;
  else if (d->eq_kind == PMX_EQ_ODE)
    r->path = entry == ENTRY_USER ? P_USER_ODE : P_ODE_BODY;
  else
    return bad("unknown eq_kind");
  if (r->path == P_ODE_BODY && d->kernel == PMX_ODE_CUSTOM) return bad("PMX_ODE_CUSTOM models are created with pmx_model_create_custom");
  if (r->path == P_ANALYTICAL && d->kernel == PMX_K_CUSTOM) return bad("PMX_K_CUSTOM models are created with pmx_model_create_user");
  if (const int32_t rc = check_desc(d, r->path, fns); rc != PMX_OK) return rc;
  pmx_model* m = r->m.get();
  m->d = *d;
  const int n_lag = count_lagged(*d);
  const uint32_t body_fns = PMX_FN_DYNAMICS | PMX_FN_OUTPUTS;
  switch (r->path) {
    case P_ANALYTICAL:
      m->dyn = binds_covariate_factors(*d);
      m->has_init = inits_from_params(*d);
      // Descriptor forms the library's own kernels do not take - lag time together with covariate-derived rate constants
      // or pm_* indexing, more than four lagged inputs - run on the user-closure walker: the derived values are written
      // out as source, every other closure is generated from the descriptor as for any user model.
      if (n_lag > pmx::kMaxLagSlots || (n_lag > 0 && (m->dyn || d->pmetrics_indexing))) {
        const bool derive = d->n_derived > 0;
        take_closure_walker(r, derive ? pmx::analytical_descriptor_source(*d) : std::string(), derive ? PMX_FN_DERIVE : 0u, true);
        r->generated("generated closures");
      }
      return PMX_OK;
    case P_ODE_BODY:
      m->has_init = inits_from_params(*d);
      if (n_lag <= pmx::kMaxLagSlots && d->n_derived == 0 && d->n_bind == 0) return PMX_OK;
      // covariate-derived parameters of a built-in diffeq body (expand/ode.rs:126-185), or more lagged inputs than the
      // state-machine kernels take: the body is written out as source, where covariates are looked up at every stage time
      m->d.kernel = PMX_ODE_CUSTOM;
      m->d.n_derived = 0;
      m->d.n_bind = 0;
      if (n_lag > pmx::kMaxLagSlots) return hand_to_general_ode_walker(r, pmx::ode_descriptor_source(*d), body_fns | PMX_FN_INIT);
      take_state_machine_body(r, pmx::ode_descriptor_source(*d), m->has_init);
      r->generated("generated diffeq body");
      return PMX_OK;
    case P_CUSTOM:
      if (n_lag > pmx::kMaxLagSlots) return hand_to_general_ode_walker(r, source, body_fns | (has_init ? PMX_FN_INIT : 0u));
      take_state_machine_body(r, source, has_init != 0);
      return PMX_OK;
    case P_USER_ANALYTICAL:
      m->user_eq = d->kernel == PMX_K_CUSTOM;
      [[fallthrough]];
    case P_USER_ODE:
      take_closure_walker(r, source, fns);
      return PMX_OK;
  }
  return PMX_OK;
}

// the model of a resolved (descriptor, closure set): compile what it needs, fix its device-side description
int32_t build(Resolved& r, pmx_model** out) {
  std::string log;
  if (r.compiled && !pmx::jit_compile(r.m->jit_spec, &r.m->jit_code, &log))
    return fail(r.fail_code, std::string("hiprtc could not compile the ") + r.fail_what + ":\n" + log);
  finish_model(r.m.get());
  *out = r.m.release();
  return PMX_OK;
}

// the translation unit build() compiles, as malloc'ed text (pmx_free_text)
int32_t text_of(const Resolved& r, char** out_text) {
  const std::string tu = pmx::jit_translation_unit(r.m->jit_spec);
  char* buf = static_cast<char*>(std::malloc(tu.size() + 1));
  if (!buf) return fail(PMX_ERR_OUT_OF_MEMORY, "malloc");
  std::memcpy(buf, tu.c_str(), tu.size() + 1);
  *out_text = buf;
  return PMX_OK;
}

template <class T, class Then>  // the shape of all five entry points: clear error, null checks, resolve, then build or text_of
int32_t with_resolved(Entry entry, const pmx_model_desc* d, const char* source, uint32_t fns, int32_t has_init, T** out,
                      const char* out_is_null, Then then) {
  pmx::clear_error();
  if (!out) return bad(out_is_null);
  *out = nullptr;
  Resolved r;
  const int32_t rc = resolve(entry, d, source, fns, has_init, &r);
  return rc != PMX_OK ? rc : then(r, out);
}

}  // namespace

extern "C" {

int32_t pmx_model_create(const pmx_model_desc* d, pmx_model** out) {
  return with_resolved(ENTRY_CREATE, d, nullptr, 0, 0, out, "null argument", build);
}
int32_t pmx_model_create_custom(const pmx_model_desc* d, const char* source, int32_t has_init, pmx_model** out) {
  return with_resolved(ENTRY_CUSTOM, d, source, 0, has_init, out, "out is null", build);
}
int32_t pmx_model_create_user(const pmx_model_desc* d, const char* source, uint32_t functions, pmx_model** out) {
  return with_resolved(ENTRY_USER, d, source, functions, 0, out, "out is null", build);
}
int32_t pmx_debug_jit_source(const pmx_model_desc* d, const char* source, int32_t has_init, char** out_text) {
  return with_resolved(ENTRY_CUSTOM, d, source, 0, has_init, out_text, "out_text is null", text_of);
}
int32_t pmx_debug_jit_source_user(const pmx_model_desc* d, const char* source, uint32_t functions, char** out_text) {
  return with_resolved(ENTRY_USER, d, source, functions, 0, out_text, "out_text is null", text_of);
}
void pmx_free_text(char* text) { std::free(text); }
void pmx_model_destroy(pmx_model* m) { delete m; }

}  // extern "C"

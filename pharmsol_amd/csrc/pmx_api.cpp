// pmx_api.cpp — the extern "C" boundary of libpmx_hip.so (include/pmx.h).
//
// No CPU compute path exists in this library: if there is no HIP device the
// entry points fail with PMX_ERR_NO_DEVICE.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "pmx_internal.hpp"
#include "pmx_structures.hpp"  // kernel_nparams()

namespace {

thread_local std::string g_err;
thread_local const char* g_kernel_name = "";

int32_t create_user_ode(const pmx_model_desc* d, const char* source, uint32_t fns, pmx_model** out);  // (after check_user_ode)

int32_t spec_solver(const pmx_model_desc* d) { return d->eq_kind == PMX_EQ_ODE ? d->ode_solver : PMX_SOLVER_RK4; }  // (JitSpec::solver)

int ode_nstates(int model) {
  static const int n[PMX_ODE_MODEL_COUNT] = {1, 2, 2, 3, 3, 4, 1};
  return (model >= 0 && model < PMX_ODE_MODEL_COUNT) ? n[model] : -1;
}
int ode_nparams(int model) {
  static const int n[PMX_ODE_MODEL_COUNT] = {1, 2, 3, 4, 5, 6, 3};
  return (model >= 0 && model < PMX_ODE_MODEL_COUNT) ? n[model] : -1;
}

// the numeric part of an ODE descriptor, the same for every pmx_model_create*: step ceiling, solver, its tolerances
int32_t check_ode_numerics(const pmx_model_desc* d) {
  if (!(d->rk4_h_max > 0.0)) return fail(PMX_ERR_INVALID_ARGUMENT, "rk4_h_max must be > 0");
  const pmx::SolverRow* solver = pmx::solver_row(d->ode_solver);
  if (!solver) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown ode_solver");
  if (solver->needs_tol && !(d->ode_rtol > 0.0 && d->ode_atol > 0.0))
    return fail(PMX_ERR_INVALID_ARGUMENT, "the adaptive solvers and checked RK4 need ode_rtol > 0 and ode_atol > 0");
  return PMX_OK;
}

// what the translation unit of a general-walker ODE model (pmx_ode.hpp) is generated from
pmx::JitSpec spec_of(const pmx_model_desc* d, const char* source, int32_t has_init) {
  pmx::JitSpec sp;
  sp.nstates = d->nstates;
  sp.nparams = d->nparams;
  sp.nout = d->nout;
  sp.ninputs = d->ndrugs > 0 ? d->ndrugs : 1;
  sp.has_init = has_init != 0;
  sp.ncov = d->n_covariates;
  sp.solver = spec_solver(d);
  sp.source = source;
  return sp;
}

// every pmx_model_create* ends here: the model's device-side description is fixed from now on
int32_t publish(std::unique_ptr<pmx_model>& m, pmx_model** out) {
  finish_model(m.get());
  *out = m.release();
  return PMX_OK;
}

}  // namespace

namespace pmx {
// the calling thread's error text / kernel name, for the other translation units of the C ABI
int32_t set_error(int32_t code, const std::string& msg) {
  g_err = msg;
  return code;
}
void set_kernel_name(const char* name) { g_kernel_name = name; }
}  // namespace pmx

// What the HOST-pointer entry points (pmx_predict, pmx_predict_batch, pmx_loglik, pmx_loglik_batch) keep between
// calls, per population: device buffers for theta / output / status (grown, never shrunk), a private stream pair and
// two pinned bounce buffers.  An NPAG loop calls these entry points thousands of times; allocating, page-locking and
// freeing per call cost ~700x the kernel (profiles/r01/pcie_inclusive.txt).  Calls on one population take turns.
struct HostWorkspace {
  std::mutex mu;
  hipStream_t compute = nullptr, copy = nullptr;
  void* d_theta = nullptr;
  void* d_out = nullptr;
  void* d_status = nullptr;
  int32_t* d_flag = nullptr;  // "any pair failed" (pmx_status_any)
  size_t theta_cap = 0, out_cap = 0, status_cap = 0;
  static constexpr size_t kBounce = 32u << 20;
  void* bounce[2] = {nullptr, nullptr};
  hipEvent_t bev[2] = {nullptr, nullptr};
  int32_t* h_flag = nullptr;  // pinned
  ~HostWorkspace() {
    if (d_theta) (void)hipFree(d_theta);
    if (d_out) (void)hipFree(d_out);
    if (d_status) (void)hipFree(d_status);
    if (d_flag) (void)hipFree(d_flag);
    for (int i = 0; i < 2; ++i) {
      if (bounce[i]) (void)hipHostFree(bounce[i]);
      if (bev[i]) (void)hipEventDestroy(bev[i]);
    }
    if (h_flag) (void)hipHostFree(h_flag);
    if (compute) (void)hipStreamDestroy(compute);
    if (copy) (void)hipStreamDestroy(copy);
  }
};

pmx_population::pmx_population() = default;
pmx_population::~pmx_population() {
  for (void* p : ll_allocs) (void)hipFree(p);
}

extern "C" {

int32_t pmx_abi_version(void) { return PMX_ABI_VERSION; }
int64_t pmx_sizeof_model_desc(void) { return static_cast<int64_t>(sizeof(pmx_model_desc)); }
int64_t pmx_sizeof_population_desc(void) { return static_cast<int64_t>(sizeof(pmx_population_desc)); }
int64_t pmx_sizeof_struct(const char* name) {
  if (!name) return -1;
#define PMX_SZ(T) \
  if (std::strcmp(name, #T) == 0) return static_cast<int64_t>(sizeof(T));
  PMX_SZ(pmx_population_desc)
  PMX_SZ(pmx_factor)
  PMX_SZ(pmx_derived)
  PMX_SZ(pmx_bind)
  PMX_SZ(pmx_out)
  PMX_SZ(pmx_model_desc)
  PMX_SZ(pmx_error_model)
  PMX_SZ(pmx_op_stream_view)
  PMX_SZ(pmx_jit_cache_counters)
#undef PMX_SZ
  return -1;
}

int32_t pmx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* pmx_last_error(void) { return g_err.c_str(); }

void pmx_debug_reload_env(void) { pmx::reload_tunables(); }
const char* pmx_last_kernel_name(void) { return g_kernel_name; }

int32_t pmx_population_create(const pmx_population_desc* desc, int32_t device, pmx_population** out) {
  g_err.clear();
  if (!out) return fail(PMX_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(PMX_ERR_NO_DEVICE, "no HIP device visible (libpmx_hip has no CPU path)");
  if (device < 0 || device >= n) return fail(PMX_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  auto pop = std::make_unique<pmx_population>();
  pop->device = device;
  std::string err;
  int32_t rc = pmx::build_host_population(desc, &pop->hp, &err);
  if (rc != PMX_OK) return fail(rc, err);
  *out = pop.release();
  return PMX_OK;
}

int32_t pmx_population_create_shard(const pmx_population_desc* desc, int64_t subject_begin, int64_t subject_end,
                                    int32_t device, pmx_population** out) {
  g_err.clear();
  if (!out) return fail(PMX_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!desc || !desc->subj_occ_off || !desc->occ_ev_off) return fail(PMX_ERR_INVALID_ARGUMENT, "null population descriptor");
  if (subject_begin < 0 || subject_end < subject_begin || subject_end > desc->n_subjects)
    return fail(PMX_ERR_INVALID_ARGUMENT, "subject range out of bounds");
  // the descriptor of subjects [begin, end): the caller's arrays addressed in place, the three CSR offset arrays re-based
  const int64_t s0 = subject_begin, s1 = subject_end;
  const int64_t o0 = desc->subj_occ_off[s0], o1 = desc->subj_occ_off[s1];
  const int64_t e0 = desc->occ_ev_off[o0], e1 = desc->occ_ev_off[o1];
  std::vector<int64_t> subj_occ(static_cast<size_t>(s1 - s0) + 1), occ_ev(static_cast<size_t>(o1 - o0) + 1), knot_off;
  for (int64_t s = s0; s <= s1; ++s) subj_occ[static_cast<size_t>(s - s0)] = desc->subj_occ_off[s] - o0;
  for (int64_t o = o0; o <= o1; ++o) occ_ev[static_cast<size_t>(o - o0)] = desc->occ_ev_off[o] - e0;
  pmx_population_desc d = *desc;
  d.n_subjects = s1 - s0;
  d.n_occasions = o1 - o0;
  d.n_events = e1 - e0;
  d.subj_occ_off = subj_occ.data();
  d.occ_ev_off = occ_ev.data();
  if (desc->occ_index) d.occ_index = desc->occ_index + o0;
  if (desc->ev_time) d.ev_time = desc->ev_time + e0;
  if (desc->ev_value) d.ev_value = desc->ev_value + e0;
  if (desc->ev_duration) d.ev_duration = desc->ev_duration + e0;
  if (desc->ev_kind) d.ev_kind = desc->ev_kind + e0;
  if (desc->ev_io) d.ev_io = desc->ev_io + e0;
  if (desc->ev_errorpoly) d.ev_errorpoly = desc->ev_errorpoly + 4 * e0;
  if (desc->ev_censor) d.ev_censor = desc->ev_censor + e0;
  const int32_t nc = desc->n_covariates;
  if (nc > 0) {
    if (!desc->cov_knot_off || !desc->cov_knot_time || !desc->cov_knot_value)
      return fail(PMX_ERR_INVALID_ARGUMENT, "covariate arrays missing");
    const int64_t c0 = o0 * nc, c1 = o1 * nc, k0 = desc->cov_knot_off[c0];
    knot_off.resize(static_cast<size_t>(c1 - c0) + 1);
    for (int64_t c = c0; c <= c1; ++c) knot_off[static_cast<size_t>(c - c0)] = desc->cov_knot_off[c] - k0;
    d.cov_knot_off = knot_off.data();
    d.cov_knot_time = desc->cov_knot_time + k0;
    d.cov_knot_value = desc->cov_knot_value + k0;
    if (desc->cov_fixed) d.cov_fixed = desc->cov_fixed + c0;
  }
  return pmx_population_create(&d, device, out);
}

void pmx_population_destroy(pmx_population* pop) {
  if (!pop) return;
  {
    DeviceGuard g;
    (void)g.enter(pop->device);
    pop->streams.clear();
    pop->ws.reset();
  }
  delete pop;
}

int64_t pmx_population_n_subjects(const pmx_population* pop) { return pop ? pop->hp.n_subjects : -1; }
int64_t pmx_population_n_observations(const pmx_population* pop) { return pop ? pop->hp.n_obs : -1; }
int64_t pmx_population_n_events(const pmx_population* pop) { return pop ? pop->hp.n_events : -1; }
int32_t pmx_population_device(const pmx_population* pop) { return pop ? pop->device : -1; }

int32_t pmx_population_observation_offsets(const pmx_population* pop, int64_t* obs_off) {
  if (!pop || !obs_off) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  std::memcpy(obs_off, pop->hp.subj_obs_off.data(), sizeof(int64_t) * pop->hp.subj_obs_off.size());
  return PMX_OK;
}

int32_t pmx_population_observation_info(const pmx_population* pop, double* time, int32_t* outeq, int64_t* subject) {
  if (!pop) return fail(PMX_ERR_INVALID_ARGUMENT, "null population");
  const auto& hp = pop->hp;
  if (time) std::memcpy(time, hp.obs_time.data(), sizeof(double) * hp.obs_time.size());
  if (outeq) std::memcpy(outeq, hp.obs_outeq.data(), sizeof(int32_t) * hp.obs_outeq.size());
  if (subject) std::memcpy(subject, hp.obs_subject.data(), sizeof(int64_t) * hp.obs_subject.size());
  return PMX_OK;
}

int32_t pmx_model_create(const pmx_model_desc* d, pmx_model** out) {
  g_err.clear();
  if (!d || !out) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (d->eq_kind == PMX_EQ_ODE && d->kernel == PMX_ODE_CUSTOM)
    return fail(PMX_ERR_INVALID_ARGUMENT, "PMX_ODE_CUSTOM models are created with pmx_model_create_custom");
  if (d->eq_kind == PMX_EQ_ANALYTICAL && d->kernel == PMX_K_CUSTOM)
    return fail(PMX_ERR_INVALID_ARGUMENT, "PMX_K_CUSTOM models are created with pmx_model_create_user");
  if (d->nstates < 1 || d->nstates > PMX_MAX_STATES) return fail(PMX_ERR_INVALID_ARGUMENT, "nstates out of range");
  if (d->ndrugs < 0 || d->ndrugs > PMX_MAX_INPUTS) return fail(PMX_ERR_INVALID_ARGUMENT, "ndrugs out of range");
  if (d->nout < 1 || d->nout > PMX_MAX_OUT) return fail(PMX_ERR_INVALID_ARGUMENT, "nout out of range");
  if (d->nparams < 0 || d->nparams > PMX_MAX_PARAMS) return fail(PMX_ERR_INVALID_ARGUMENT, "nparams out of range");
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES)
    return fail(PMX_ERR_INVALID_ARGUMENT, "n_covariates out of range");
  if (d->n_derived < 0 || d->n_derived > PMX_MAX_DERIVED) return fail(PMX_ERR_INVALID_ARGUMENT, "n_derived out of range");
  for (int i = 0; i < d->n_derived; ++i) {
    const pmx_derived& dd = d->derived[i];
    if (dd.src_param < 0 || dd.src_param >= d->nparams) return fail(PMX_ERR_INVALID_ARGUMENT, "derived.src_param out of range");
    if (dd.n_factors < 0 || dd.n_factors > PMX_MAX_FACTORS) return fail(PMX_ERR_INVALID_ARGUMENT, "derived.n_factors out of range");
    for (int k = 0; k < dd.n_factors; ++k)
      if (dd.f[k].op != PMX_F_NONE && (dd.f[k].cov < 0 || dd.f[k].cov >= d->n_covariates))
        return fail(PMX_ERR_INVALID_ARGUMENT, "derived factor covariate out of range");
  }
  auto m = std::make_unique<pmx_model>();
  m->d = *d;
  const int pm = d->pmetrics_indexing ? 1 : 0;
  bool to_user_walker = false, ode_many_lags = false;
  if (d->eq_kind == PMX_EQ_ANALYTICAL) {
    if (d->kernel < 0 || d->kernel >= PMX_K_ANALYTICAL_COUNT) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown analytical kernel");
    static const int kNS[12] = {1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4};  // AnalyticalKernel::state_count analysis.rs:259-270
    if (d->nstates < kNS[d->kernel] + pm) return fail(PMX_ERR_INVALID_ARGUMENT, "model has fewer states than its structure");
    const int np = pmx::kernel_nparams(d->kernel);
    if (d->n_bind == 0 && d->nparams < np) return fail(PMX_ERR_INVALID_ARGUMENT, "too few parameters for the structure");
    if (d->n_bind != 0 && d->n_bind != np) return fail(PMX_ERR_INVALID_ARGUMENT, "n_bind must equal the structure's parameter count");
    for (int j = 0; j < d->n_bind; ++j) {
      const pmx_bind& b = d->bind[j];
      if (b.src == PMX_SRC_PRIMARY) {
        if (b.index < 0 || b.index >= d->nparams) return fail(PMX_ERR_INVALID_ARGUMENT, "bind index out of range");
      } else if (b.src == PMX_SRC_DERIVED) {
        if (b.index < 0 || b.index >= d->n_derived) return fail(PMX_ERR_INVALID_ARGUMENT, "bind derived index out of range");
        if (d->derived[b.index].n_factors > 0) m->dyn = true;
      } else
        return fail(PMX_ERR_INVALID_ARGUMENT, "bind.src must be PRIMARY or DERIVED");
    }
    int n_lag = 0;
    for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
      if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams)
        return fail(PMX_ERR_INVALID_ARGUMENT, "lag_param / fa_param out of range");
      if (d->lag_param[i] >= 0) ++n_lag;
    }
    // Descriptor forms the library's own kernels do not take - lag time together with covariate-derived rate constants
    // or pm_* indexing, more than four lagged inputs - run on the user-closure walker instead (pmx_analytical.hpp): the
    // derived values are written out as source, every other closure is generated from the descriptor as for any user model.
    to_user_walker = n_lag > pmx::kMaxLagSlots || (n_lag > 0 && (m->dyn || pm));
  } else if (d->eq_kind == PMX_EQ_ODE) {
    if (ode_nstates(d->kernel) < 0) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown ODE model");
    if (d->nstates < ode_nstates(d->kernel)) return fail(PMX_ERR_INVALID_ARGUMENT, "model has fewer states than its diffeq");
    if (d->nparams < ode_nparams(d->kernel)) return fail(PMX_ERR_INVALID_ARGUMENT, "too few parameters for the diffeq");
    if (const int32_t rc = check_ode_numerics(d); rc != PMX_OK) return rc;
    if (pm) return fail(PMX_ERR_INVALID_ARGUMENT, "pm_* indexing is a wrapper of the analytical structures (analytical/mod.rs:62-90): it does not apply to ODE models");
    if (d->n_bind != 0 && d->n_bind != ode_nparams(d->kernel))
      return fail(PMX_ERR_INVALID_ARGUMENT, "n_bind must equal the diffeq's parameter count");
    for (int j = 0; j < d->n_bind; ++j) {
      const pmx_bind& b = d->bind[j];
      if (b.src == PMX_SRC_PRIMARY ? (b.index < 0 || b.index >= d->nparams)
                                   : (b.src != PMX_SRC_DERIVED || b.index < 0 || b.index >= d->n_derived))
        return fail(PMX_ERR_INVALID_ARGUMENT, "bind entry out of range");
    }
    {
      int n_lag = 0;
      for (int i = 0; i < PMX_MAX_INPUTS; ++i) n_lag += d->lag_param[i] >= 0;
      ode_many_lags = n_lag > pmx::kMaxLagSlots;  // (the state-machine kernels keep four lag cursors: the general ODE walker takes over)
    }
    for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
      if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams)
        return fail(PMX_ERR_INVALID_ARGUMENT, "lag_param / fa_param out of range");
      if (d->bolus_dest[i] >= d->nstates || d->infusion_dest[i] >= d->nstates)
        return fail(PMX_ERR_INVALID_ARGUMENT, "route destination out of range");
    }
  } else
    return fail(PMX_ERR_INVALID_ARGUMENT, "unknown eq_kind");
  for (int o = 0; o < d->nout; ++o) {
    const pmx_out& oo = d->out[o];
    if (oo.state < 0 || oo.state >= d->nstates) return fail(PMX_ERR_INVALID_ARGUMENT, "out.state out of range");
    if (oo.vol_src == PMX_SRC_PRIMARY && (oo.vol_index < 0 || oo.vol_index >= d->nparams))
      return fail(PMX_ERR_INVALID_ARGUMENT, "out.vol_index out of range");
    if (oo.vol_src == PMX_SRC_DERIVED && (oo.vol_index < 0 || oo.vol_index >= d->n_derived))
      return fail(PMX_ERR_INVALID_ARGUMENT, "out.vol_index (derived) out of range");
  }
  for (int i = 0; i < PMX_MAX_STATES; ++i) {
    if (d->init_param[i] >= d->nparams) return fail(PMX_ERR_INVALID_ARGUMENT, "init_param out of range");
    if (d->init_param[i] >= 0 && i < d->nstates) m->has_init = true;
  }
  if (to_user_walker) {
    pmx::JitSpec sp;
    sp.analytical = true;
    sp.fns = d->n_derived > 0 ? static_cast<uint32_t>(PMX_FN_DERIVE) : 0u;
    sp.desc = *d;
    sp.source = d->n_derived > 0 ? pmx::analytical_descriptor_source(*d) : std::string();
    std::string log;
    m->jit_spec = sp;
    if (!pmx::jit_compile(sp, &m->jit_code, &log))
      return fail(PMX_ERR_HIP, "hiprtc could not compile the generated closures:\n" + log);
    m->custom = true;
    m->dyn = false;
    m->user_fns = sp.fns;
    m->user_lag = true;
    m->has_init = true;  // (RESET ops always carry the occasion-index flag; the policy's init may be empty)
  }
  if (ode_many_lags) {  // built-in diffeq body, more than four lagged inputs: body written out as source, the general ODE walker
    pmx_model_desc dd = *d;
    dd.kernel = PMX_ODE_CUSTOM;
    dd.n_derived = 0;
    dd.n_bind = 0;
    const std::string src = pmx::ode_descriptor_source(*d);
    return create_user_ode(&dd, src.c_str(), PMX_FN_DYNAMICS | PMX_FN_OUTPUTS | PMX_FN_INIT, out);
  }
  if (d->eq_kind == PMX_EQ_ODE && (d->n_derived > 0 || d->n_bind > 0)) {
    // covariate-derived parameters of a built-in diffeq body (expand/ode.rs:126-185): the body is written out as source
    // and takes the run-time-compiled path, where covariates are looked up on the device at every stage time
    pmx_model_desc dd = *d;
    dd.kernel = PMX_ODE_CUSTOM;
    dd.n_derived = 0;
    dd.n_bind = 0;
    std::string log;
    m->jit_spec = spec_of(d, pmx::ode_descriptor_source(*d).c_str(), m->has_init);
    if (!pmx::jit_compile(m->jit_spec, &m->jit_code, &log))
      return fail(PMX_ERR_HIP, "hiprtc could not compile the generated diffeq body:\n" + log);
    m->d = dd;
    m->custom = true;
  }
  return publish(m, out);
}

}  // extern "C"

namespace {
int32_t check_custom_desc(const pmx_model_desc* d, const char* source) {
  if (!d || !source) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (d->eq_kind != PMX_EQ_ODE || d->kernel != PMX_ODE_CUSTOM)
    return fail(PMX_ERR_INVALID_ARGUMENT, "custom models need eq_kind = PMX_EQ_ODE and kernel = PMX_ODE_CUSTOM");
  if (d->nstates < 1 || d->nstates > PMX_MAX_STATES) return fail(PMX_ERR_INVALID_ARGUMENT, "nstates out of range");
  if (d->ndrugs < 0 || d->ndrugs > PMX_MAX_INPUTS) return fail(PMX_ERR_INVALID_ARGUMENT, "ndrugs out of range");
  if (d->nout < 1 || d->nout > PMX_MAX_OUT) return fail(PMX_ERR_INVALID_ARGUMENT, "nout out of range");
  if (d->nparams < 1 || d->nparams > PMX_MAX_PARAMS) return fail(PMX_ERR_INVALID_ARGUMENT, "nparams out of range");
  if (const int32_t rc = check_ode_numerics(d); rc != PMX_OK) return rc;
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES)
    return fail(PMX_ERR_INVALID_ARGUMENT, "n_covariates out of range");
  if (d->n_derived != 0 || d->n_bind != 0 || d->pmetrics_indexing)
    return fail(PMX_ERR_INVALID_ARGUMENT, "derived-parameter descriptors / pm indexing do not apply to custom ODE bodies (compute them in the body)");
  int n_lag = 0;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
    if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams)
      return fail(PMX_ERR_INVALID_ARGUMENT, "lag_param / fa_param out of range");
    if (d->bolus_dest[i] >= d->nstates) return fail(PMX_ERR_INVALID_ARGUMENT, "route destination out of range");
    n_lag += d->lag_param[i] >= 0;
  }
  (void)n_lag;  // (more than four lagged inputs: pmx_model_create_custom hands the model to the general ODE walker)
  return PMX_OK;
}
}  // namespace

extern "C" {

int32_t pmx_model_create_custom(const pmx_model_desc* d, const char* source, int32_t has_init, pmx_model** out) {
  g_err.clear();
  if (!out) return fail(PMX_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  const int32_t rc = check_custom_desc(d, source);
  if (rc != PMX_OK) return rc;
  {
    int n_lag = 0;
    for (int i = 0; i < PMX_MAX_INPUTS; ++i) n_lag += d->lag_param[i] >= 0;
    if (n_lag > pmx::kMaxLagSlots)  // the state-machine kernels keep four lag cursors: the general ODE walker sorts any number
      return create_user_ode(d, source, PMX_FN_DYNAMICS | PMX_FN_OUTPUTS | (has_init ? PMX_FN_INIT : 0u), out);
  }
  auto m = std::make_unique<pmx_model>();
  m->d = *d;
  m->custom = true;
  m->has_init = has_init != 0;
  std::string log;
  m->jit_spec = spec_of(d, source, has_init);
  if (!pmx::jit_compile(m->jit_spec, &m->jit_code, &log))
    return fail(PMX_ERR_INVALID_ARGUMENT, "hiprtc could not compile the model source:\n" + log);
  return publish(m, out);
}

int32_t pmx_debug_jit_source(const pmx_model_desc* d, const char* source, int32_t has_init, char** out_text) {
  g_err.clear();
  if (!out_text) return fail(PMX_ERR_INVALID_ARGUMENT, "out_text is null");
  *out_text = nullptr;
  const int32_t rc = check_custom_desc(d, source);
  if (rc != PMX_OK) return rc;
  const std::string tu = pmx::jit_translation_unit(spec_of(d, source, has_init));
  char* buf = static_cast<char*>(std::malloc(tu.size() + 1));
  if (!buf) return fail(PMX_ERR_OUT_OF_MEMORY, "malloc");
  std::memcpy(buf, tu.c_str(), tu.size() + 1);
  *out_text = buf;
  return PMX_OK;
}

void pmx_free_text(char* text) { std::free(text); }

}  // extern "C"

namespace {
// Analytical model with user closures: what of the descriptor must hold (pmx.h "user closures for either back-end")
int32_t check_user_analytical(const pmx_model_desc* d, const char* source, uint32_t fns) {
  if (!d || !source) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (d->nstates < 1 || d->nstates > PMX_MAX_STATES) return fail(PMX_ERR_INVALID_ARGUMENT, "nstates out of range");
  if (d->ndrugs < 1 || d->ndrugs > PMX_MAX_INPUTS) return fail(PMX_ERR_INVALID_ARGUMENT, "ndrugs out of range (1..8 for a model with user closures)");
  if (d->nout < 1 || d->nout > PMX_MAX_OUT) return fail(PMX_ERR_INVALID_ARGUMENT, "nout out of range");
  if (d->nparams < 1 || d->nparams > PMX_MAX_PARAMS) return fail(PMX_ERR_INVALID_ARGUMENT, "nparams out of range");
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES) return fail(PMX_ERR_INVALID_ARGUMENT, "n_covariates out of range");
  if (d->n_derived < 0 || d->n_derived > PMX_MAX_USER_DERIVED) return fail(PMX_ERR_INVALID_ARGUMENT, "n_derived out of range");
  if (d->n_derived > 0 && !(fns & PMX_FN_DERIVE)) return fail(PMX_ERR_INVALID_ARGUMENT, "n_derived > 0 needs PMX_FN_DERIVE (desc.derived[] is not read for user models)");
  if (d->pmetrics_indexing && d->kernel == PMX_K_CUSTOM)
    return fail(PMX_ERR_INVALID_ARGUMENT, "pm_* indexing wraps a built-in structure: it does not apply to a user propagator (pmx_eq)");
  if (fns & PMX_FN_DYNAMICS) return fail(PMX_ERR_INVALID_ARGUMENT, "PMX_FN_DYNAMICS belongs to ODE models");
  if (d->kernel == PMX_K_CUSTOM) {
    if (!(fns & PMX_FN_EQ)) return fail(PMX_ERR_INVALID_ARGUMENT, "kernel = PMX_K_CUSTOM needs PMX_FN_EQ");
  } else {
    if (fns & PMX_FN_EQ) return fail(PMX_ERR_INVALID_ARGUMENT, "PMX_FN_EQ needs kernel = PMX_K_CUSTOM");
    if (d->kernel < 0 || d->kernel >= PMX_K_ANALYTICAL_COUNT) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown analytical kernel");
    static const int kNS[12] = {1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4};
    if (d->nstates < kNS[d->kernel] + (d->pmetrics_indexing ? 1 : 0)) return fail(PMX_ERR_INVALID_ARGUMENT, "model has fewer states than its structure");
    const int np = pmx::kernel_nparams(d->kernel);
    if (d->n_bind == 0 && d->nparams < np) return fail(PMX_ERR_INVALID_ARGUMENT, "too few parameters for the structure");
    if (d->n_bind != 0 && d->n_bind != np) return fail(PMX_ERR_INVALID_ARGUMENT, "n_bind must equal the structure's parameter count");
    for (int j = 0; j < d->n_bind; ++j) {
      const pmx_bind& b = d->bind[j];
      if (b.src == PMX_SRC_PRIMARY ? (b.index < 0 || b.index >= d->nparams)
                                   : (b.src != PMX_SRC_DERIVED || b.index < 0 || b.index >= d->n_derived))
        return fail(PMX_ERR_INVALID_ARGUMENT, "bind entry out of range");
    }
  }
  for (int i = 0; i < PMX_MAX_INPUTS; ++i)
    if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams)
      return fail(PMX_ERR_INVALID_ARGUMENT, "lag_param / fa_param out of range");
  for (int i = 0; i < PMX_MAX_STATES; ++i)
    if (d->init_param[i] >= d->nparams) return fail(PMX_ERR_INVALID_ARGUMENT, "init_param out of range");
  if (!(fns & PMX_FN_OUTPUTS))
    for (int o = 0; o < d->nout; ++o) {
      const pmx_out& oo = d->out[o];
      if (oo.state < 0 || oo.state >= d->nstates) return fail(PMX_ERR_INVALID_ARGUMENT, "out.state out of range");
      if (oo.vol_src == PMX_SRC_PRIMARY && (oo.vol_index < 0 || oo.vol_index >= d->nparams))
        return fail(PMX_ERR_INVALID_ARGUMENT, "out.vol_index out of range");
      if (oo.vol_src == PMX_SRC_DERIVED && (oo.vol_index < 0 || oo.vol_index >= d->n_derived))
        return fail(PMX_ERR_INVALID_ARGUMENT, "out.vol_index (derived) out of range");
    }
  return PMX_OK;
}
// ODE model with user closures beyond the dynamics (pmx.h "user closures for either back-end", ODE models)
int32_t check_user_ode(const pmx_model_desc* d, const char* source, uint32_t fns) {
  if (!d || !source) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (d->kernel != PMX_ODE_CUSTOM) return fail(PMX_ERR_INVALID_ARGUMENT, "ODE models with user closures need kernel = PMX_ODE_CUSTOM");
  const bool dyn = (fns & PMX_FN_DYNAMICS) != 0, dynb = (fns & PMX_FN_DYNAMICS_BOLUS) != 0;
  if (dyn == dynb) return fail(PMX_ERR_INVALID_ARGUMENT, "ODE models define pmx_dynamics OR pmx_dynamics_bolus (PMX_FN_DYNAMICS | PMX_FN_DYNAMICS_BOLUS)");
  if (!(fns & PMX_FN_OUTPUTS)) return fail(PMX_ERR_INVALID_ARGUMENT, "ODE models define pmx_outputs (PMX_FN_OUTPUTS)");
  if (fns & (PMX_FN_SEQ_EQ | PMX_FN_EQ)) return fail(PMX_ERR_INVALID_ARGUMENT, "PMX_FN_SEQ_EQ / PMX_FN_EQ belong to analytical models");
  if (d->nstates < 1 || d->nstates > PMX_MAX_STATES) return fail(PMX_ERR_INVALID_ARGUMENT, "nstates out of range");
  if (d->ndrugs < 1 || d->ndrugs > PMX_MAX_INPUTS) return fail(PMX_ERR_INVALID_ARGUMENT, "ndrugs out of range (1..8 for a model with user closures)");
  if (d->nout < 1 || d->nout > PMX_MAX_OUT) return fail(PMX_ERR_INVALID_ARGUMENT, "nout out of range");
  if (d->nparams < 1 || d->nparams > PMX_MAX_PARAMS) return fail(PMX_ERR_INVALID_ARGUMENT, "nparams out of range");
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES) return fail(PMX_ERR_INVALID_ARGUMENT, "n_covariates out of range");
  if (d->n_derived < 0 || d->n_derived > PMX_MAX_USER_DERIVED) return fail(PMX_ERR_INVALID_ARGUMENT, "n_derived out of range");
  if (d->n_derived > 0 && !(fns & PMX_FN_DERIVE)) return fail(PMX_ERR_INVALID_ARGUMENT, "n_derived > 0 needs PMX_FN_DERIVE (desc.derived[] is not read for user models)");
  if (d->n_bind != 0 || d->pmetrics_indexing) return fail(PMX_ERR_INVALID_ARGUMENT, "bind[] / pm indexing do not apply to ODE models with user closures");
  if (const int32_t rc = check_ode_numerics(d); rc != PMX_OK) return rc;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
    if (d->lag_param[i] >= d->nparams || d->fa_param[i] >= d->nparams)
      return fail(PMX_ERR_INVALID_ARGUMENT, "lag_param / fa_param out of range");
    if (d->bolus_dest[i] >= d->nstates) return fail(PMX_ERR_INVALID_ARGUMENT, "route destination out of range");
  }
  for (int i = 0; i < PMX_MAX_STATES; ++i)
    if (d->init_param[i] >= d->nparams) return fail(PMX_ERR_INVALID_ARGUMENT, "init_param out of range");
  return PMX_OK;
}
pmx::JitSpec user_spec_of(const pmx_model_desc* d, const char* source, uint32_t fns) {
  pmx::JitSpec sp;
  sp.analytical = d->eq_kind == PMX_EQ_ANALYTICAL;
  sp.ode_user = d->eq_kind == PMX_EQ_ODE;
  sp.fns = fns;
  sp.desc = *d;
  sp.solver = spec_solver(d);
  sp.source = source;
  return sp;
}
int32_t create_user_ode(const pmx_model_desc* d, const char* source, uint32_t fns, pmx_model** out) {
  const int32_t rc = check_user_ode(d, source, fns);
  if (rc != PMX_OK) return rc;
  auto m = std::make_unique<pmx_model>();
  m->d = *d;
  m->custom = true;
  m->user_ode = true;
  m->user_fns = fns;
  m->user_lag = (fns & PMX_FN_ROUTE_LAG) != 0;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) m->user_lag |= d->lag_param[i] >= 0;
  m->has_init = true;  // (RESET ops always carry the occasion-index flag; the policy's init may be empty)
  std::string log;
  m->jit_spec = user_spec_of(d, source, fns);
  if (!pmx::jit_compile(m->jit_spec, &m->jit_code, &log))
    return fail(PMX_ERR_INVALID_ARGUMENT, "hiprtc could not compile the model source:\n" + log);
  return publish(m, out);
}
}  // namespace

extern "C" {

int32_t pmx_model_create_user(const pmx_model_desc* d, const char* source, uint32_t functions, pmx_model** out) {
  g_err.clear();
  if (!out) return fail(PMX_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!d) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (d->eq_kind == PMX_EQ_ODE) {
    if ((functions & ~static_cast<uint32_t>(PMX_FN_INIT)) == (PMX_FN_DYNAMICS | PMX_FN_OUTPUTS) && d->n_derived == 0)
      return pmx_model_create_custom(d, source, (functions & PMX_FN_INIT) ? 1 : 0, out);  // theta-indexed lag / fa: the state-machine kernels
    return create_user_ode(d, source, functions, out);
  }
  if (d->eq_kind != PMX_EQ_ANALYTICAL) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown eq_kind");
  const int32_t rc = check_user_analytical(d, source, functions);
  if (rc != PMX_OK) return rc;
  auto m = std::make_unique<pmx_model>();
  m->d = *d;
  m->custom = true;
  m->user_fns = functions;
  m->user_eq = d->kernel == PMX_K_CUSTOM;
  m->user_lag = (functions & PMX_FN_ROUTE_LAG) != 0;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) m->user_lag |= d->lag_param[i] >= 0;
  m->has_init = true;  // (RESET ops always carry the occasion-index flag; the policy's init may be empty)
  std::string log;
  m->jit_spec = user_spec_of(d, source, functions);
  if (!pmx::jit_compile(m->jit_spec, &m->jit_code, &log))
    return fail(PMX_ERR_INVALID_ARGUMENT, "hiprtc could not compile the model source:\n" + log);
  return publish(m, out);
}

int32_t pmx_debug_jit_source_user(const pmx_model_desc* d, const char* source, uint32_t functions, char** out_text) {
  g_err.clear();
  if (!out_text) return fail(PMX_ERR_INVALID_ARGUMENT, "out_text is null");
  *out_text = nullptr;
  if (!d) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (d->eq_kind == PMX_EQ_ODE && (functions & ~static_cast<uint32_t>(PMX_FN_INIT)) == (PMX_FN_DYNAMICS | PMX_FN_OUTPUTS) &&
      d->n_derived == 0)
    return pmx_debug_jit_source(d, source, (functions & PMX_FN_INIT) ? 1 : 0, out_text);
  const int32_t rc = d->eq_kind == PMX_EQ_ODE ? check_user_ode(d, source, functions) : check_user_analytical(d, source, functions);
  if (rc != PMX_OK) return rc;
  const std::string tu = pmx::jit_translation_unit(user_spec_of(d, source, functions));
  char* buf = static_cast<char*>(std::malloc(tu.size() + 1));
  if (!buf) return fail(PMX_ERR_OUT_OF_MEMORY, "malloc");
  std::memcpy(buf, tu.c_str(), tu.size() + 1);
  *out_text = buf;
  return PMX_OK;
}

void pmx_model_destroy(pmx_model* m) { delete m; }

}  // extern "C"

namespace {

// ---- host-pointer forms -------------------------------------------------------------------------------------------
int32_t ws_get(pmx_population* pop, HostWorkspace** out) {
  std::lock_guard<std::mutex> lock(pop->mu);
  if (!pop->ws) {
    auto ws = std::make_unique<HostWorkspace>();
    PMX_HIP(hipStreamCreateWithFlags(&ws->compute, hipStreamNonBlocking));
    PMX_HIP(hipStreamCreateWithFlags(&ws->copy, hipStreamNonBlocking));
    PMX_HIP(hipMalloc(reinterpret_cast<void**>(&ws->d_flag), sizeof(int32_t)));
    PMX_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->h_flag), sizeof(int32_t), hipHostMallocDefault));
    for (int i = 0; i < 2; ++i) {
      PMX_HIP(hipHostMalloc(&ws->bounce[i], HostWorkspace::kBounce, hipHostMallocDefault));
      PMX_HIP(hipEventCreateWithFlags(&ws->bev[i], hipEventDisableTiming));
    }
    pop->ws = std::move(ws);
  }
  *out = pop->ws.get();
  return PMX_OK;
}

int32_t ws_reserve(void** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return PMX_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = need > 0 ? ((need + (1u << 20) - 1) >> 20) << 20 : (1u << 20);  // whole MiB
  PMX_HIP(hipMalloc(p, want));
  *cap = want;
  return PMX_OK;
}

bool is_pinned_host(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an ordinary malloc'ed pointer: "invalid value", not an error of ours)
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// rows x row_bytes from a dense device buffer to host rows `dst_pitch` apart, after everything enqueued on ws->compute.
// Page-locked destinations (pmx_host_alloc, hipHostMalloc, hipHostRegister) take ONE DMA at link rate; pageable ones go
// through the two pinned bounce buffers, the DMA of one piece overlapping the CPU copy of the previous one.
int32_t ws_copy_out(HostWorkspace* ws, void* dst, size_t dst_pitch, const void* src, size_t row_bytes, size_t rows) {
  if (rows == 0 || row_bytes == 0) {
    PMX_HIP(hipStreamSynchronize(ws->compute));
    return PMX_OK;
  }
  if (is_pinned_host(dst)) {
    if (dst_pitch == row_bytes)
      PMX_HIP(hipMemcpyAsync(dst, src, row_bytes * rows, hipMemcpyDeviceToHost, ws->compute));
    else
      PMX_HIP(hipMemcpy2DAsync(dst, dst_pitch, src, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, ws->compute));
    PMX_HIP(hipStreamSynchronize(ws->compute));
    return PMX_OK;
  }
  PMX_HIP(hipStreamSynchronize(ws->compute));
  const size_t total = row_bytes * rows;
  const size_t piece = HostWorkspace::kBounce;
  const size_t n_pieces = (total + piece - 1) / piece;
  auto land = [&](size_t k) {  // bounce[k % 2] -> the caller's rows
    const size_t off = k * piece, len = (off + piece <= total) ? piece : total - off;
    const char* b = static_cast<const char*>(ws->bounce[k % 2]);
    if (dst_pitch == row_bytes) {
      std::memcpy(static_cast<char*>(dst) + off, b, len);
      return;
    }
    size_t done = 0;
    while (done < len) {  // split at row ends
      const size_t at = off + done, r = at / row_bytes, c = at % row_bytes;
      const size_t n = (row_bytes - c < len - done) ? row_bytes - c : len - done;
      std::memcpy(static_cast<char*>(dst) + r * dst_pitch + c, b + done, n);
      done += n;
    }
  };
  for (size_t k = 0; k < n_pieces; ++k) {
    const size_t off = k * piece, len = (off + piece <= total) ? piece : total - off;
    PMX_HIP(hipMemcpyAsync(ws->bounce[k % 2], static_cast<const char*>(src) + off, len, hipMemcpyDeviceToHost, ws->copy));
    PMX_HIP(hipEventRecord(ws->bev[k % 2], ws->copy));
    if (k > 0) {
      PMX_HIP(hipEventSynchronize(ws->bev[(k - 1) % 2]));
      land(k - 1);
    }
  }
  PMX_HIP(hipEventSynchronize(ws->bev[(n_pieces - 1) % 2]));
  land(n_pieces - 1);
  return PMX_OK;
}

// Every exit path of a host-pointer entry point leaves nothing in flight: the caller may free or reuse theta and its
// (possibly page-locked) outputs as soon as the call returns - also when it returns an error half-way - and the next
// call reuses the workspace buffers.
struct WsDrain {
  HostWorkspace* ws;
  ~WsDrain() {
    (void)hipStreamSynchronize(ws->compute);
    (void)hipStreamSynchronize(ws->copy);
  }
};

// the per-pair status bytes: "did any pair fail" comes back as ONE flag reduced on the device (the array itself is only
// copied when the caller asked for it: 100 MB for C3)
int32_t ws_finish_status(HostWorkspace* ws, uint8_t* status, size_t n_status, bool* any_failed) {
  PMX_HIP(hipMemsetAsync(ws->d_flag, 0, sizeof(int32_t), ws->compute));
  PMX_HIP(pmx::launch_status_any(static_cast<const uint8_t*>(ws->d_status), static_cast<int64_t>(n_status), ws->d_flag, ws->compute));
  PMX_HIP(hipMemcpyAsync(ws->h_flag, ws->d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, ws->compute));
  if (status) {
    const int32_t rc = ws_copy_out(ws, status, n_status, ws->d_status, n_status, 1);
    if (rc != PMX_OK) return rc;
  } else {
    PMX_HIP(hipStreamSynchronize(ws->compute));
  }
  *any_failed = *ws->h_flag != 0;
  return PMX_OK;
}

int32_t predict_host(const pmx_model* model, const pmx_population* cpop, const double* theta, int64_t P, int batch,
                     double* pred, int64_t ld, uint8_t* status) {
  g_err.clear();
  if (!model || !cpop || !theta || !pred) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  const int64_t S = pop->hp.n_subjects, NO = pop->hp.n_obs;
  if (!batch && (P <= 0 || ld < P)) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_pred >= n_support");
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  HostWorkspace* ws = nullptr;
  int32_t rc = ws_get(pop, &ws);
  if (rc != PMX_OK) return rc;
  std::lock_guard<std::mutex> turn(ws->mu);
  WsDrain drain{ws};
  const int64_t rows_theta = batch ? S : P;
  const int64_t Pd = batch ? 1 : P;  // the device matrix is dense; the caller's padding columns are never touched
  const size_t n_status = static_cast<size_t>(batch ? S : S * P);
  const size_t theta_bytes = static_cast<size_t>(rows_theta) * model->d.nparams * sizeof(double);
  const size_t pred_bytes = static_cast<size_t>(NO) * Pd * sizeof(double);
  if ((rc = ws_reserve(&ws->d_theta, &ws->theta_cap, theta_bytes)) != PMX_OK) return rc;
  if ((rc = ws_reserve(&ws->d_out, &ws->out_cap, pred_bytes)) != PMX_OK) return rc;
  if ((rc = ws_reserve(&ws->d_status, &ws->status_cap, n_status)) != PMX_OK) return rc;
  PMX_HIP(hipMemcpyAsync(ws->d_theta, theta, theta_bytes, hipMemcpyHostToDevice, ws->compute));
  if (n_status > 0) PMX_HIP(hipMemsetAsync(ws->d_status, 0, n_status, ws->compute));
  rc = enqueue(model, pop, static_cast<const double*>(ws->d_theta), P, batch, static_cast<double*>(ws->d_out), Pd,
               static_cast<uint8_t*>(ws->d_status), ws->compute);
  if (rc != PMX_OK) return rc;
  bool any_failed = false;
  if ((rc = ws_finish_status(ws, status, n_status, &any_failed)) != PMX_OK) return rc;
  if ((rc = ws_copy_out(ws, pred, static_cast<size_t>(batch ? 1 : ld) * sizeof(double), ws->d_out,
                        static_cast<size_t>(Pd) * sizeof(double), static_cast<size_t>(NO))) != PMX_OK)
    return rc;
  if (any_failed)
    return fail(PMX_ERR_PAIR_FAILED, "at least one (subject, support point) pair failed; see the status array");
  return PMX_OK;
}

// ll[s][p] (matrix shape) or ll[s] (batch shape: subject s with theta row s, likelihood/mod.rs:119-177)
int32_t loglik_host(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em, const double* theta,
                    int64_t P, int batch, double* ll, int64_t ld_ll, uint8_t* status) {
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  const int64_t S = pop->hp.n_subjects;
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  HostWorkspace* ws = nullptr;
  int32_t rc = ws_get(pop, &ws);
  if (rc != PMX_OK) return rc;
  std::lock_guard<std::mutex> turn(ws->mu);
  WsDrain drain{ws};
  const int64_t Pd = batch ? 1 : P;
  const size_t theta_bytes = static_cast<size_t>(batch ? S : P) * model->d.nparams * sizeof(double);
  const size_t ll_bytes = static_cast<size_t>(S) * Pd * sizeof(double);
  const size_t n_status = static_cast<size_t>(S) * Pd;
  if ((rc = ws_reserve(&ws->d_theta, &ws->theta_cap, theta_bytes)) != PMX_OK) return rc;
  if ((rc = ws_reserve(&ws->d_out, &ws->out_cap, ll_bytes)) != PMX_OK) return rc;
  if ((rc = ws_reserve(&ws->d_status, &ws->status_cap, n_status)) != PMX_OK) return rc;
  PMX_HIP(hipMemcpyAsync(ws->d_theta, theta, theta_bytes, hipMemcpyHostToDevice, ws->compute));
  if (n_status > 0) PMX_HIP(hipMemsetAsync(ws->d_status, 0, n_status, ws->compute));
  const int32_t* d_sigma_err = nullptr;
  LLRequest req{em, static_cast<double*>(ws->d_out), Pd, &d_sigma_err};
  rc = enqueue(model, pop, static_cast<const double*>(ws->d_theta), P, batch, static_cast<double*>(ws->d_out), Pd,
               static_cast<uint8_t*>(ws->d_status), ws->compute, &req);
  if (rc != PMX_OK) return rc;
  if (d_sigma_err) {  // ErrorModelError::NegativeSigma / NonFiniteSigma (error_model.rs:1073-1077), found on the device
    PMX_HIP(hipMemcpyAsync(ws->h_flag, d_sigma_err, sizeof(int32_t), hipMemcpyDeviceToHost, ws->compute));
    PMX_HIP(hipStreamSynchronize(ws->compute));
    const int32_t n_bad = *ws->h_flag;
    if (n_bad > 0)
      return fail(PMX_ERR_ERROR_MODEL, "NegativeSigma / NonFiniteSigma for " + std::to_string(n_bad) + " observation(s)");
  }
  bool any_failed = false;
  if ((rc = ws_finish_status(ws, status, n_status, &any_failed)) != PMX_OK) return rc;
  if ((rc = ws_copy_out(ws, ll, static_cast<size_t>(batch ? 1 : ld_ll) * sizeof(double), ws->d_out,
                        static_cast<size_t>(Pd) * sizeof(double), static_cast<size_t>(S))) != PMX_OK)
    return rc;
  if (any_failed) {
    if (batch) {
      // log_likelihood_batch maps a failed subject to -inf instead of failing the call (likelihood/mod.rs:137-140):
      // the status array names them, the caller's row is overwritten here
      std::vector<uint8_t> hst(n_status);
      PMX_HIP(hipMemcpy(hst.data(), ws->d_status, n_status, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n_status; ++i)
        if (hst[i] != PMX_PAIR_OK) ll[i] = -std::numeric_limits<double>::infinity();
      return PMX_OK;
    }
    return fail(PMX_ERR_PAIR_FAILED, "at least one (subject, support point) pair failed; see the status array");
  }
  return PMX_OK;
}

}  // namespace

extern "C" {

int32_t pmx_predict(const pmx_model* model, const pmx_population* pop, const double* theta, int64_t n_support,
                    double* pred, int64_t ld_pred, uint8_t* status) {
  return predict_host(model, pop, theta, n_support, 0, pred, ld_pred, status);
}

int32_t pmx_predict_batch(const pmx_model* model, const pmx_population* pop, const double* theta, double* pred,
                          uint8_t* status) {
  return predict_host(model, pop, theta, 1, 1, pred, 1, status);
}

int32_t pmx_predict_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                           int64_t n_support, double* d_pred, int64_t ld_pred, uint8_t* d_status, void* stream) {
  g_err.clear();
  if (!model || !cpop || !d_theta || !d_pred) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_pred < n_support) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_pred >= n_support");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  return enqueue(model, pop, d_theta, n_support, 0, d_pred, ld_pred, d_status, stream);
}

// the model of a *_stats_device call integrates with PMX_SOLVER_AUTO (checked before any device is touched)
static bool stats_model_ok(const pmx_model* model) {
  return model->d.eq_kind == PMX_EQ_ODE && model->d.ode_solver == PMX_SOLVER_AUTO;
}

int32_t pmx_predict_stats_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 int64_t n_support, double* d_pred, int64_t ld_pred, uint8_t* d_status, void* stream,
                                 uint32_t* d_stats) {
  g_err.clear();
  if (!model) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!stats_model_ok(model)) return fail(PMX_ERR_INVALID_ARGUMENT, "solver statistics exist for PMX_SOLVER_AUTO models only");
  if (!cpop || !d_theta || !d_pred || !d_stats) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_pred < n_support) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_pred >= n_support");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  return enqueue(model, pop, d_theta, n_support, 0, d_pred, ld_pred, d_status, stream, nullptr, -1, d_stats);
}

int32_t pmx_predict_batch_stats_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                       double* d_pred, uint8_t* d_status, void* stream, uint32_t* d_stats) {
  g_err.clear();
  if (!model) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!stats_model_ok(model)) return fail(PMX_ERR_INVALID_ARGUMENT, "solver statistics exist for PMX_SOLVER_AUTO models only");
  if (!cpop || !d_theta || !d_pred || !d_stats) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  return enqueue(model, pop, d_theta, 1, 1, d_pred, 1, d_status, stream, nullptr, -1, d_stats);
}

int32_t pmx_time_predict_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                int64_t n_support, double* d_pred, int64_t ld_pred, int32_t reps, void* stream,
                                double* ms_per_pass) {
  g_err.clear();
  if (!model || !cpop || !d_theta || !d_pred || !ms_per_pass) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_pred < n_support || reps < 1) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support, ld_pred or reps out of range");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t rc = enqueue(model, pop, d_theta, n_support, 0, d_pred, ld_pred, nullptr, stream);
  if (rc != PMX_OK) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PMX_HIP(hipEventCreate(&e0));
  PMX_HIP(hipEventCreate(&e1));
  PMX_HIP(hipEventRecord(e0, st));
  for (int32_t i = 0; i < reps && rc == PMX_OK; ++i) rc = enqueue(model, pop, d_theta, n_support, 0, d_pred, ld_pred, nullptr, stream);
  if (rc == PMX_OK) {
    float ms = 0.0f;
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) rc = fail(PMX_ERR_HIP, hipGetErrorString(e));
    *ms_per_pass = static_cast<double>(ms) / reps;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

int32_t pmx_predict_state_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 int64_t n_support, int32_t state, double* d_out, int64_t ld_out, uint8_t* d_status,
                                 void* stream) {
  g_err.clear();
  if (!model || !cpop || !d_theta || !d_out) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_out < n_support) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_out >= n_support");
  if (state < 0 || state >= model->d.nstates) return fail(PMX_ERR_INVALID_ARGUMENT, "state out of range");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  return enqueue(model, pop, d_theta, n_support, 0, d_out, ld_out, d_status, stream, nullptr, state);
}

int32_t pmx_predict_batch_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 double* d_pred, uint8_t* d_status, void* stream) {
  g_err.clear();
  if (!model || !cpop || !d_theta || !d_pred) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  return enqueue(model, pop, d_theta, 1, 1, d_pred, 1, d_status, stream);
}

}  // extern "C"

// ---- host-side introspection ---------------------------------------------------
namespace {
struct DebugOwner {
  pmx::HostPopulation hp;
  pmx::StreamPlan sp;
};

// the stream plan of a (population, model) pair exactly as a launch would build it: same key, same class-plan switches
int32_t debug_plan(const pmx_population_desc* pop, const pmx_model_desc* model, pmx::HostPopulation* hp, pmx::StreamPlan* sp,
                   pmx::CompileKey* key) {
  pmx_model* m = nullptr;
  int32_t rc = pmx_model_create(model, &m);
  if (rc != PMX_OK) return rc;
  std::unique_ptr<pmx_model> mg(m);
  std::string err;
  rc = pmx::build_host_population(pop, hp, &err);
  if (rc != PMX_OK) return fail(rc, err);
  const pmx::Tunables tun = pmx::tunables();
  *key = key_for(m, tun, hp->has_infusions);
  rc = pmx::plan_stream(*hp, *key, tun.cls, sp, &err);
  return rc != PMX_OK ? fail(rc, err) : PMX_OK;
}
}  // namespace

extern "C" {

int32_t pmx_debug_compile(const pmx_population_desc* pop, const pmx_model_desc* model, pmx_op_stream_view* out) {
  g_err.clear();
  if (!pop || !model || !out) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof(*out));
  auto own = std::make_unique<DebugOwner>();
  pmx::CompileKey key;
  const int32_t rc = debug_plan(pop, model, &own->hp, &own->sp, &key);
  if (rc != PMX_OK) return rc;
  const pmx::OpStream& os = own->sp.os;
  out->n_subjects = own->hp.n_subjects;
  out->n_ops = os.n_ops;
  out->n_cov = own->hp.n_cov;
  out->n_rate = os.key.n_rate;
  out->max_input_used = os.max_input_used;
  out->max_outeq = own->hp.max_outeq;
  out->subj_op_off = os.subj_op_off.data();
  out->op_meta = os.op_meta.data();
  out->op_a = os.op_a.data();
  out->op_b = os.op_b.data();
  out->op_n = os.op_n.empty() ? nullptr : os.op_n.data();
  out->op_rate = os.op_rate.empty() ? nullptr : os.op_rate.data();
  out->op_cov = os.op_cov.empty() ? nullptr : os.op_cov.data();
  out->subj_order = os.subj_order.data();
  out->owner = own.release();
  return PMX_OK;
}

int32_t pmx_debug_class_plan(const pmx_population_desc* pop, const pmx_model_desc* model, int64_t* counts) {
  g_err.clear();
  if (!pop || !model || !counts) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  pmx::HostPopulation hp;
  pmx::StreamPlan sp;
  pmx::CompileKey key;
  const int32_t rc = debug_plan(pop, model, &hp, &sp, &key);
  if (rc != PMX_OK) return rc;
  for (int i = 0; i < 5; ++i) counts[i] = 0;
  counts[3] = hp.n_subjects;
  if (key.class_g > 0) {
    const pmx::ClassPlan& cp = sp.cp;
    counts[0] = cp.n_chunks_exact;
    counts[1] = cp.n_chunks - cp.n_chunks_exact;
    counts[2] = cp.n_classed_subjects;
    counts[3] = static_cast<int64_t>(cp.generic_subjects.size());
    counts[4] = cp.G;
  }
  return PMX_OK;
}

void pmx_debug_free(pmx_op_stream_view* view) {
  if (!view || !view->owner) return;
  delete static_cast<DebugOwner*>(view->owner);
  std::memset(view, 0, sizeof(*view));
}

}  // extern "C"

// ---- fused log-likelihood -------------------------------------------------------------------------
extern "C" {

int32_t pmx_loglik_device(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                          const double* d_theta, int64_t n_support, double* d_ll, int64_t ld_ll, uint8_t* d_status,
                          void* stream) {
  g_err.clear();
  if (!model || !cpop || !em || !d_theta || !d_ll) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_ll < n_support) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_ll >= n_support");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  LLRequest req{em, d_ll, ld_ll};
  // pred is not written in log-likelihood mode; pass the ll buffer as a non-null placeholder
  return enqueue(model, pop, d_theta, n_support, 0, d_ll, ld_ll, d_status, stream, &req);
}

int32_t pmx_loglik(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em, const double* theta,
                   int64_t n_support, double* ll, int64_t ld_ll, uint8_t* status) {
  g_err.clear();
  if (!model || !cpop || !em || !theta || !ll) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0 || ld_ll < n_support) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_ll >= n_support");
  return loglik_host(model, cpop, em, theta, n_support, 0, ll, ld_ll, status);
}

int32_t pmx_loglik_batch(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em, const double* theta,
                         double* ll, uint8_t* status) {
  g_err.clear();
  if (!model || !cpop || !em || !theta || !ll) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  return loglik_host(model, cpop, em, theta, 1, 1, ll, 1, status);
}

int32_t pmx_loglik_batch_device(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                                const double* d_theta, double* d_ll, uint8_t* d_status, void* stream) {
  g_err.clear();
  if (!model || !cpop || !em || !d_theta || !d_ll) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  DeviceGuard g;
  PMX_HIP(g.enter(pop->device));
  LLRequest req{em, d_ll, 1};
  return enqueue(model, pop, d_theta, 1, 1, d_ll, 1, d_status, stream, &req);
}

int64_t pmx_recommended_ld(int64_t n_support) { return n_support <= 0 ? 0 : (n_support + 15) / 16 * 16; }

int32_t pmx_measure_write_ceiling(double* d_buf, int64_t n_doubles, int32_t reps, void* stream, double* gb_per_s) {
  g_err.clear();
  if (!d_buf || !gb_per_s || n_doubles < 2 || reps < 1) return fail(PMX_ERR_INVALID_ARGUMENT, "bad argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PMX_HIP(hipEventCreate(&e0));
  PMX_HIP(hipEventCreate(&e1));
  hipError_t e = hipSuccess;
  float best_ms = 0.0f;
  for (int shape = 0; shape < 4 && e == hipSuccess; ++shape) {  // the best of four store shapes (pmx_util.hip)
    e = pmx::launch_fill_linear(d_buf, n_doubles, 0.0, stream, shape);  // untimed
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int32_t i = 0; i < reps && e == hipSuccess; ++i) e = pmx::launch_fill_linear(d_buf, n_doubles, 0.0, stream, shape);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess && (shape == 0 || ms < best_ms)) best_ms = ms;
  }
  const float ms = best_ms;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return fail(PMX_ERR_HIP, hipGetErrorString(e));
  *gb_per_s = static_cast<double>(n_doubles / 2 * 16) * reps / (static_cast<double>(ms) * 1.0e-3) / 1.0e9;
  return PMX_OK;
}

int32_t pmx_host_alloc(int64_t bytes, void** out) {
  g_err.clear();
  if (!out || bytes < 0) return fail(PMX_ERR_INVALID_ARGUMENT, "bad argument");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(PMX_ERR_NO_DEVICE, "no HIP device visible");
  PMX_HIP(hipHostMalloc(out, static_cast<size_t>(bytes > 0 ? bytes : 1), hipHostMallocDefault));
  return PMX_OK;
}

void pmx_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

}  // extern "C"
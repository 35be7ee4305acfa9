// pmx_api.cpp — the extern "C" boundary of libpmx_hip.so (include/pmx.h): version and sizes, error text, populations, the
// device-pointer entry points, debug views and measurement helpers.  Model creation: pmx_model.cpp; the host-pointer
// entry points: pmx_host.cpp.
//
// No CPU compute path exists in this library: if there is no HIP device the
// entry points fail with PMX_ERR_NO_DEVICE.
#include <cstring>
#include <initializer_list>

#include "pmx_internal.hpp"

namespace {

thread_local std::string g_err;
thread_local const char* g_kernel_name = "";

}  // namespace

namespace pmx {
// the calling thread's error text / kernel name, for the other translation units of the C ABI
int32_t set_error(int32_t code, const std::string& msg) {
  g_err = msg;
  return code;
}
void set_kernel_name(const char* name) { g_kernel_name = name; }
}  // namespace pmx

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

int64_t pmx_population_n_profiles(const pmx_population* pop) {
  if (!pop) return -1;
  host_profiles(const_cast<pmx_population*>(pop));
  return pop->profiles.n();
}

int32_t pmx_population_profile_info(const pmx_population* pop, int64_t* subject, int64_t* occasion, int32_t* outeq,
                                    int64_t* n_rows) {
  if (!pop) return fail(PMX_ERR_INVALID_ARGUMENT, "null population");
  host_profiles(const_cast<pmx_population*>(pop));
  const auto& pr = pop->profiles;
  const size_t n = static_cast<size_t>(pr.n());
  if (subject) std::memcpy(subject, pr.subject.data(), sizeof(int64_t) * n);
  if (occasion) std::memcpy(occasion, pr.occasion.data(), sizeof(int64_t) * n);
  if (outeq) std::memcpy(outeq, pr.outeq.data(), sizeof(int32_t) * n);
  if (n_rows)
    for (size_t k = 0; k < n; ++k) n_rows[k] = pr.off[k + 1] - pr.off[k];
  return PMX_OK;
}

}  // extern "C"

// ---- device-pointer forms -------------------------------------------------------------------------------------------
namespace {

// The front of every *_device entry point: its argument checks in the order given (the first that fails names the
// refusal), then the population's device for the length of the call.
struct Arg {
  bool ok;
  const char* text;
};
constexpr const char* kNull = "null argument";
struct DeviceCall {
  DeviceGuard guard;
  pmx_population* pop = nullptr;
  int32_t begin(const pmx_population* cpop, std::initializer_list<Arg> args) {
    pmx::clear_error();
    for (const Arg& a : args)
      if (!a.ok) return fail(PMX_ERR_INVALID_ARGUMENT, a.text);
    pop = const_cast<pmx_population*>(cpop);
    PMX_HIP(guard.enter(pop->device));
    return PMX_OK;
  }
};
bool matrix_ok(int64_t n_support, int64_t ld) { return n_support > 0 && ld >= n_support; }

// method, window, threshold and metric bits of an exposure call (exposure_refusal, pmx_internal.hpp)
Arg exposure_request(int32_t method, const double* window, uint32_t metrics) {
  const char* why = exposure_refusal(method, window, metrics);
  return {why == nullptr, why};
}

// the model of a *_stats_device call integrates with PMX_SOLVER_AUTO (checked before any other pointer, and before any device is touched)
Arg stats_model(const pmx_model* model) {
  return {model && model->d.eq_kind == PMX_EQ_ODE && model->d.ode_solver == PMX_SOLVER_AUTO,
          model ? "solver statistics exist for PMX_SOLVER_AUTO models only" : kNull};
}

// milliseconds between two points of a stream
struct StreamTimer {
  hipStream_t st;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit StreamTimer(void* stream) : st(static_cast<hipStream_t>(stream)) {}
  ~StreamTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t start() {
    hipError_t e = e0 ? hipSuccess : hipEventCreate(&e0);
    if (e == hipSuccess && !e1) e = hipEventCreate(&e1);
    return e == hipSuccess ? hipEventRecord(e0, st) : e;
  }
  hipError_t stop(float* ms) {
    hipError_t e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    return e == hipSuccess ? hipEventElapsedTime(ms, e0, e1) : e;
  }
};

}  // namespace

extern "C" {

int32_t pmx_predict_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                           int64_t n_support, double* d_pred, int64_t ld_pred, uint8_t* d_status, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{model && cpop && d_theta && d_pred, kNull},
                                    {matrix_ok(n_support, ld_pred), "n_support must be > 0 and ld_pred >= n_support"}});
  return rc != PMX_OK ? rc : enqueue(model, c.pop, d_theta, n_support, 0, d_pred, ld_pred, d_status, stream);
}

int32_t pmx_predict_batch_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 double* d_pred, uint8_t* d_status, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{model && cpop && d_theta && d_pred, kNull}});
  return rc != PMX_OK ? rc : enqueue(model, c.pop, d_theta, 1, 1, d_pred, 1, d_status, stream);
}

int32_t pmx_predict_stats_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 int64_t n_support, double* d_pred, int64_t ld_pred, uint8_t* d_status, void* stream,
                                 uint32_t* d_stats) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {stats_model(model), {cpop && d_theta && d_pred && d_stats, kNull},
                                    {matrix_ok(n_support, ld_pred), "n_support must be > 0 and ld_pred >= n_support"}});
  return rc != PMX_OK ? rc : enqueue(model, c.pop, d_theta, n_support, 0, d_pred, ld_pred, d_status, stream, nullptr, -1, d_stats);
}

int32_t pmx_predict_batch_stats_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                       double* d_pred, uint8_t* d_status, void* stream, uint32_t* d_stats) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {stats_model(model), {cpop && d_theta && d_pred && d_stats, kNull}});
  return rc != PMX_OK ? rc : enqueue(model, c.pop, d_theta, 1, 1, d_pred, 1, d_status, stream, nullptr, -1, d_stats);
}

int32_t pmx_predict_state_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                 int64_t n_support, int32_t state, double* d_out, int64_t ld_out, uint8_t* d_status,
                                 void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{model && cpop && d_theta && d_out, kNull},
                                    {matrix_ok(n_support, ld_out), "n_support must be > 0 and ld_out >= n_support"},
                                    {model && state >= 0 && state < model->d.nstates, "state out of range"}});
  return rc != PMX_OK ? rc : enqueue(model, c.pop, d_theta, n_support, 0, d_out, ld_out, d_status, stream, nullptr, state);
}

int32_t pmx_loglik_device(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                          const double* d_theta, int64_t n_support, double* d_ll, int64_t ld_ll, uint8_t* d_status,
                          void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{model && cpop && em && d_theta && d_ll, kNull},
                                    {matrix_ok(n_support, ld_ll), "n_support must be > 0 and ld_ll >= n_support"}});
  if (rc != PMX_OK) return rc;
  LLRequest req{em, d_ll, ld_ll};
  // pred is not written in log-likelihood mode; pass the ll buffer as a non-null placeholder
  return enqueue(model, c.pop, d_theta, n_support, 0, d_ll, ld_ll, d_status, stream, &req);
}

int32_t pmx_loglik_batch_device(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                                const double* d_theta, double* d_ll, uint8_t* d_status, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{model && cpop && em && d_theta && d_ll, kNull}});
  if (rc != PMX_OK) return rc;
  LLRequest req{em, d_ll, 1};
  return enqueue(model, c.pop, d_theta, 1, 1, d_ll, 1, d_status, stream, &req);
}

// the reductions of a matrix pmx_loglik_device wrote (pmx_mixture.hip)
int32_t pmx_mixture_loglik_device(const pmx_population* cpop, const double* d_ll, int64_t n_support, int64_t ld_ll,
                                  const double* d_w, double* d_lpyl, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{cpop && d_ll && d_w && d_lpyl, kNull},
                                    {matrix_ok(n_support, ld_ll), "n_support must be > 0 and ld_ll >= n_support"}});
  if (rc != PMX_OK) return rc;
  PMX_HIP(pmx::launch_mixture_rows(d_ll, c.pop->hp.n_subjects, n_support, ld_ll, d_w, d_lpyl, stream));
  return PMX_OK;
}

int64_t pmx_dfunction_scratch_doubles(int64_t n_subjects, int64_t n_cand) {
  if (n_subjects <= 0 || n_cand <= 0) return -1;
  return pmx::dfunction_tiles(n_subjects, n_cand) * n_cand;
}

int32_t pmx_dfunction_device(const pmx_population* cpop, const double* d_ll, int64_t n_cand, int64_t ld_ll,
                             const double* d_lpyl, double* d_scratch, double* d_D, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{cpop && d_ll && d_lpyl && d_scratch && d_D, kNull},
                                    {matrix_ok(n_cand, ld_ll), "n_cand must be > 0 and ld_ll >= n_cand"}});
  if (rc != PMX_OK) return rc;
  PMX_HIP(pmx::launch_dfunction(d_ll, c.pop->hp.n_subjects, n_cand, ld_ll, d_lpyl, d_scratch, d_D, stream));
  return PMX_OK;
}

// the posterior, and the summaries of a matrix pmx_predict_device wrote (pmx_posterior.hip)
int32_t pmx_posterior_device(const pmx_population* cpop, const double* d_ll, int64_t n_support, int64_t ld_ll,
                             const double* d_w, const double* d_lpyl, double* d_post, int64_t ld_post, void* stream) {
  DeviceCall c;
  const int32_t rc = c.begin(cpop, {{cpop && d_ll && d_w && d_lpyl && d_post, kNull},
                                    {matrix_ok(n_support, ld_ll), "n_support must be > 0 and ld_ll >= n_support"},
                                    {ld_post >= n_support, "ld_post must be >= n_support"}});
  if (rc != PMX_OK) return rc;
  PMX_HIP(pmx::launch_posterior_rows(d_ll, c.pop->hp.n_subjects, n_support, ld_ll, d_w, d_lpyl, d_post, ld_post, stream));
  return PMX_OK;
}

int32_t pmx_summarize_predictions_device(const pmx_population* cpop, const double* d_pred, int64_t n_support, int64_t ld_pred,
                                         const double* d_w, const double* d_ll, int64_t ld_ll, const double* d_lpyl,
                                         double* d_mean, double* d_median, void* stream) {
  DeviceCall c;
  int32_t rc = c.begin(cpop, {{cpop && d_pred && d_w, kNull},
                              {d_mean || d_median, "d_mean and d_median are both null: nothing to compute"},
                              {(d_ll == nullptr) == (d_lpyl == nullptr), "d_ll and d_lpyl go together: both (posterior) or neither (population)"},
                              {matrix_ok(n_support, ld_pred), "n_support must be > 0 and ld_pred >= n_support"},
                              {!d_ll || ld_ll >= n_support, "ld_ll must be >= n_support"}});
  if (rc != PMX_OK) return rc;
  if (d_ll && (rc = resident_obs_off(c.pop)) != PMX_OK) return rc;
  const pmx::SummaryArgs a{d_pred, c.pop->hp.n_obs, n_support, ld_pred, d_w, d_ll, ld_ll, d_lpyl, c.pop->d_subj_obs_off,
                           c.pop->hp.n_subjects, c.pop->max_subject_rows, d_mean, d_median};
  PMX_HIP(pmx::launch_summary_rows(a, stream));
  return PMX_OK;
}

// the exposure metrics of a matrix pmx_predict_device wrote, and their attainment (pmx_exposure.hip)
int32_t pmx_exposure_device(const pmx_population* cpop, const double* d_pred, int64_t n_support, int64_t ld_pred,
                            int32_t method, const double* window, uint32_t metrics, double* d_out, int64_t ld_out,
                            void* stream) {
  DeviceCall c;
  int32_t rc = c.begin(cpop, {{cpop && d_pred && d_out, kNull},
                              {matrix_ok(n_support, ld_pred), "n_support must be > 0 and ld_pred >= n_support"},
                              {ld_out >= n_support, "ld_out must be >= n_support"},
                              exposure_request(method, window, metrics)});
  if (rc != PMX_OK) return rc;
  if ((rc = resident_profiles(c.pop)) != PMX_OK) return rc;
  const auto& pr = c.pop->profiles;
  const ExposureWindow win(window);
  const pmx::ExposureArgs a{d_pred, n_support, ld_pred, pr.d_off, pr.d_row, pr.d_time, pr.n(), method,
                            win.a, win.b, win.threshold, metrics, d_out, ld_out};
  PMX_HIP(pmx::launch_exposure(a, stream));
  return PMX_OK;
}

int32_t pmx_attainment_device(const pmx_population* cpop, const double* d_metric, int64_t n_support, int64_t ld_metric,
                              const double* d_target, const double* d_w, const double* d_ll, int64_t ld_ll,
                              const double* d_lpyl, double* d_pta, double* d_mean, void* stream) {
  DeviceCall c;
  int32_t rc = c.begin(cpop, {{cpop && d_metric && d_w, kNull},
                              {d_pta || d_mean, "d_pta and d_mean are both null: nothing to compute"},
                              {!d_pta || d_target, "d_pta needs d_target"},
                              {(d_ll == nullptr) == (d_lpyl == nullptr), "d_ll and d_lpyl go together: both (posterior) or neither (population)"},
                              {matrix_ok(n_support, ld_metric), "n_support must be > 0 and ld_metric >= n_support"},
                              {!d_ll || ld_ll >= n_support, "ld_ll must be >= n_support"}});
  if (rc != PMX_OK) return rc;
  if ((rc = resident_profiles(c.pop)) != PMX_OK) return rc;
  const auto& pr = c.pop->profiles;
  const pmx::AttainArgs a{d_metric, pr.n(), n_support, ld_metric, d_target, d_w, d_ll, ld_ll, d_lpyl, pr.d_subject, d_pta, d_mean};
  PMX_HIP(pmx::launch_attainment(a, stream));
  return PMX_OK;
}

int32_t pmx_time_predict_device(const pmx_model* model, const pmx_population* cpop, const double* d_theta,
                                int64_t n_support, double* d_pred, int64_t ld_pred, int32_t reps, void* stream,
                                double* ms_per_pass) {
  DeviceCall c;
  int32_t rc = c.begin(cpop, {{model && cpop && d_theta && d_pred && ms_per_pass, kNull},
                              {matrix_ok(n_support, ld_pred) && reps >= 1, "n_support, ld_pred or reps out of range"}});
  if (rc != PMX_OK) return rc;
  rc = enqueue(model, c.pop, d_theta, n_support, 0, d_pred, ld_pred, nullptr, stream);  // untimed
  if (rc != PMX_OK) return rc;
  StreamTimer timer(stream);
  PMX_HIP(timer.start());
  for (int32_t i = 0; i < reps && rc == PMX_OK; ++i) rc = enqueue(model, c.pop, d_theta, n_support, 0, d_pred, ld_pred, nullptr, stream);
  if (rc != PMX_OK) return rc;
  float ms = 0.0f;
  const hipError_t e = timer.stop(&ms);
  *ms_per_pass = static_cast<double>(ms) / reps;
  return e != hipSuccess ? fail(PMX_ERR_HIP, hipGetErrorString(e)) : PMX_OK;
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

// ---- measurement helpers ------------------------------------------------------------------------------------------
extern "C" {

int64_t pmx_recommended_ld(int64_t n_support) { return n_support <= 0 ? 0 : (n_support + 15) / 16 * 16; }

int32_t pmx_measure_write_ceiling(double* d_buf, int64_t n_doubles, int32_t reps, void* stream, double* gb_per_s) {
  g_err.clear();
  if (!d_buf || !gb_per_s || n_doubles < 2 || reps < 1) return fail(PMX_ERR_INVALID_ARGUMENT, "bad argument");
  // events and launches belong on the buffer's device, whichever one is current in the caller
  DeviceGuard guard;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, d_buf) == hipSuccess) {
    PMX_HIP(guard.enter(attr.device));
  } else {
    (void)hipGetLastError();  // (a pointer the runtime cannot place: stay on the current device)
  }
  // The fills store 16 bytes per lane: an odd n_doubles leaves one double behind them.  One 8-byte store writes it,
  // outside the timed loops: with each shape's untimed first fill, and once more after the last timed repetition.
  double* const tail = (n_doubles & 1) ? d_buf + (n_doubles - 1) : nullptr;
  StreamTimer timer(stream);
  hipError_t e = hipSuccess;
  float best_ms = 0.0f;
  for (int shape = 0; shape < 4 && e == hipSuccess; ++shape) {  // the best of four store shapes (pmx_util.hip)
    e = pmx::launch_fill_linear(d_buf, n_doubles, 0.0, stream, shape);  // untimed
    if (e == hipSuccess && tail) e = pmx::launch_fill_one(tail, 0.0, stream);
    if (e == hipSuccess) e = timer.start();
    for (int32_t i = 0; i < reps && e == hipSuccess; ++i) e = pmx::launch_fill_linear(d_buf, n_doubles, 0.0, stream, shape);
    float ms = 0.0f;
    if (e == hipSuccess) e = timer.stop(&ms);
    if (e == hipSuccess && (shape == 0 || ms < best_ms)) best_ms = ms;
  }
  if (e == hipSuccess && tail) e = pmx::launch_fill_one(tail, 0.0, stream);
  if (e != hipSuccess) return fail(PMX_ERR_HIP, hipGetErrorString(e));
  *gb_per_s = static_cast<double>(n_doubles / 2 * 16) * reps / (static_cast<double>(best_ms) * 1.0e-3) / 1.0e9;
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

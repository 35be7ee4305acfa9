// pmx_internal.hpp — what the translation units of the C ABI share: the opaque handles of include/pmx.h, the device
// stream of a (population, model flavour) pair and the developer switches.
//   pmx_api.cpp     error text, populations, device-pointer entry points, debug views, measurement helpers
//   pmx_model.cpp   model creation: path table, descriptor checks, resolve, build; the hiprtc source views
//   pmx_host.cpp    host-pointer entry points and the workspace they keep on the population
//   pmx_stream.cpp  DeviceStream: plan (pmx_plan.cpp plan_stream), upload, log-likelihood slots
//   pmx_launch.cpp  compile key, route decision, enqueue
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pmx.h"
#include "pmx_compile.hpp"
#include "pmx_jit.hpp"
#include "pmx_kernels.hpp"

namespace pmx {

// the calling thread's error text (pmx_last_error) and kernel name (pmx_last_kernel_name): pmx_api.cpp
int32_t set_error(int32_t code, const std::string& msg);
void set_kernel_name(const char* name);
inline void clear_error() { (void)set_error(PMX_OK, std::string()); }  // the first act of every entry point

// Developer switches (INTEGRATION.md "environment switches").  Read ONCE, at the first call that needs them: a
// std::getenv per launch is measurable on the 11 us C2 pass.  pmx_debug_reload_env() re-reads them (tuning scripts
// and tests that flip a switch inside one process).  A launch takes ONE snapshot (tunables()) and passes it down.
struct Tunables {
  bool disable_ladder = false, disable_classing = false, ll_old = false;
  bool disable_steps = false, disable_dyn3 = false;  // set at all - even to 0 or empty - switches the walker off
  int32_t steps_per_trip = 0, grid_min_p = 0, cpb = 0;
  ClassTunables cls;
  int32_t prop_slots = -1, dyn_tile = 0;
  // code-object cache (pmx_jit_cache.cpp): PMX_JIT_CACHE=0 off, PMX_JIT_CACHE_ENTRIES, PMX_JIT_CACHE_DIR (null: no disk
  // level; the text is interned and never freed, so that a snapshot stays a plain copy)
  bool jit_cache = true;
  int32_t jit_cache_entries = 64;
  const char* jit_cache_dir = nullptr;
  void load();
};
Tunables tunables();
void reload_tunables();

}  // namespace pmx

inline int32_t fail(int32_t code, const std::string& msg) { return pmx::set_error(code, msg); }

#define PMX_HIP(call)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(e_ == hipErrorOutOfMemory ? PMX_ERR_OUT_OF_MEMORY : PMX_ERR_HIP,                 \
                  std::string(#call) + ": " + hipGetErrorString(e_));                              \
  } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
  int prev = -1;
  bool active = false;
  hipError_t enter(int dev) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev != dev) {
      e = hipSetDevice(dev);
      active = (e == hipSuccess);
    }
    return e;
  }
  ~DeviceGuard() {
    if (active) (void)hipSetDevice(prev);
  }
};

// What a launch decision reads of a stream: scalars of its StreamPlan, nothing that lives on the device.
struct StreamFacts {
  int32_t max_input_used = -1;
  int64_t max_lagb_per_list = 0;
  int64_t n_chunks = 0, n_chunks_exact = 0, n_generic = 0, n_classed_subjects = 0;
  bool has_steps = false;      // fused step records exist (the lean walker can serve the stream)
  bool has_kfac = false;       // op_kfac rows exist (the matrix-free walker can)
  bool has_chunk_hdr = false;  // prog_rec + chunk_hdr exist (pmx_analytical_classed_ll can)
  int32_t prop_slots = 0;      // LDS slots the kernel decodes the stream's propagator-cache codes with (0 = none used)
  bool no_rates = false, eig_reuse = false;  // StreamPlan
  double prop_reuse_fraction = 0.0;
};
inline StreamFacts facts_of(const pmx::StreamPlan& sp, const pmx::CompileKey& key) {
  StreamFacts f;
  f.max_input_used = sp.os.max_input_used;
  f.max_lagb_per_list = sp.os.max_lagb_per_list;
  f.n_chunks = sp.cp.n_chunks;
  f.n_chunks_exact = sp.cp.n_chunks_exact;
  f.n_generic = sp.cp.n_chunks > 0 ? static_cast<int64_t>(sp.cp.generic_subjects.size()) : 0;
  f.n_classed_subjects = sp.cp.n_chunks > 0 ? sp.cp.n_classed_subjects : 0;
  f.has_steps = !sp.step_rec.empty();
  f.has_kfac = !sp.op_kfac.empty();
  f.has_chunk_hdr = !sp.chunk_hdr.empty();
  // the stream's codes were written for key.prop_cache_slots slots; the kernel decodes them with the same number
  f.prop_slots = sp.os.prop_cache_used > 0 ? key.prop_cache_slots : 0;
  f.no_rates = sp.no_rates;
  f.eig_reuse = sp.eig_reuse;
  f.prop_reuse_fraction = sp.prop_reuse_fraction;
  return f;
}

struct DeviceStream {
  pmx::CompileKey key;
  StreamFacts f;
  pmx::DevOps dev{};
  pmx::DevClassPlan cls{};
  pmx::DevSteps steps{};  // fused step programs of the lean generic walker (analytical streams without lag / covariates)
  // Sigma tables of the log-likelihood, per set of error models.  They are filled ON THE DEVICE
  // (pmx_util.hip pmx_ll_prepare_*), stream-ordered before the kernel that reads them: an optimiser that changes
  // gamma / lambda every call pays two ~10 us kernels, not a host pass over every observation plus a 40 MB upload.
  // A small LRU of slots; uses of one slot are chained through its event so that a slot is never rewritten while a
  // kernel on another stream still reads it.
  struct LLCache {
    std::vector<pmx_error_model> em;
    double* d_obs = nullptr;   // [n_obs][4]
    double* d_cobs = nullptr;  // classed blocks
    int32_t* d_err = nullptr;  // invalid-sigma counter of the last fill
    hipEvent_t ev = nullptr;   // last use (fill or read) of this slot
    int64_t stamp = 0;         // LRU
    int32_t host_users = 0;    // host threads between "picked" and "launched"
  };
  std::deque<LLCache> ll_cache;  // (deque: slots handed out by pointer must survive later push_backs)
  int64_t ll_stamp = 0;
  const int32_t* d_chunk_nobs = nullptr;     // [n_chunks] observations per member of the chunk's class
  const int64_t* d_chunk_obs_off = nullptr;  // [n_chunks] offsets into a slot's cobs
  int64_t cobs_size = 0;
  std::vector<void*> allocs;
  ~DeviceStream() {
    for (void* p : allocs) (void)hipFree(p);
    for (auto& c : ll_cache)
      if (c.ev) (void)hipEventDestroy(c.ev);
  }
};

struct HostWorkspace;  // pmx_host.cpp: what the host-pointer entry points keep between calls

struct pmx_population {
  int device = 0;
  pmx::HostPopulation hp;
  std::mutex mu;
  std::unique_ptr<HostWorkspace> ws;  // created by the first host-pointer call
  // what the log-likelihood tables are computed from, uploaded at the first pmx_loglik* call
  bool ll_ready = false;
  const double* d_obs_y = nullptr;
  const int32_t* d_obs_outeq = nullptr;
  const double* d_obs_poly = nullptr;
  const int8_t* d_obs_cens = nullptr;
  uint32_t valued_outeq_mask = 0;  // bit q: some observation on output q carries a value
  bool any_censored = false;
  std::vector<void*> ll_allocs;
  // the rows of each subject, for the summaries of a prediction matrix (pmx_posterior.hip): uploaded at the first such
  // call (resident_obs_off), freed with ll_allocs
  const int64_t* d_subj_obs_off = nullptr;
  int64_t max_subject_rows = 0;
  // the profile table, for the exposure metrics (pmx_exposure.hip): the prediction rows of every (subject, occasion,
  // outeq) that has one, ordered by subject, occasion position, outeq.  Built on the host at the first call that asks
  // for it (host_profiles), uploaded at the first device call (resident_profiles), freed with ll_allocs.
  struct Profiles {
    bool built = false;
    std::vector<int64_t> off;       // [n + 1] into row / time
    std::vector<int64_t> row;       // [n_obs] prediction rows in profile order
    std::vector<double> time;       // [n_obs] their times
    std::vector<int64_t> subject, occasion;  // [n]
    std::vector<int32_t> outeq;     // [n]
    const int64_t* d_off = nullptr;
    const int64_t* d_row = nullptr;
    const double* d_time = nullptr;
    const int64_t* d_subject = nullptr;
    bool resident = false;
    int64_t n() const { return static_cast<int64_t>(subject.size()); }
  } profiles;
  std::vector<std::unique_ptr<DeviceStream>> streams;  // one per model flavour, built lazily
  pmx_population();
  ~pmx_population();  // (pmx_host.cpp, where HostWorkspace is complete; pmx_population_destroy too)
};

struct pmx_model {
  pmx_model_desc d;
  bool dyn = false;  // kernel parameters depend on covariates
  bool has_init = false;
  // custom (hiprtc) models: the code object and its per-device modules
  bool custom = false;
  uint32_t user_fns = 0;  // PMX_FN_* the user's source defines (pmx_model_create_user)
  bool user_lag = false, user_eq = false;  // user model: any lag closure (user's or descriptor's) / own propagator
  bool user_ode = false;                   // ODE model on the general walker (pmx_ode_user.hpp): lag / fa / derive closures, bolus[]
  // what every launch of the model passes to its kernel, fixed at creation (pmx_launch.cpp finish_model)
  pmx::DevModel dev{};
  bool vol_has_factors = false;  // some output's volume is a derived value with covariate factors (not lane-constant)
  std::vector<char> jit_code;
  pmx::JitSpec jit_spec;  // what jit_code was compiled from (the big-lists build below is made from it on demand)
  mutable std::vector<char> jit_code_big;  // closure walkers: the PMX_USER_BIG_LISTS build, compiled at the first launch on a
                                           // population with more than 64 lagged boluses in one occasion (pmx_userlag.hpp)
  mutable std::mutex jit_mu;
  mutable std::map<int, pmx::JitModule> jit_modules;
  mutable std::map<int, pmx::JitModule> jit_modules_big;
  ~pmx_model() {
    for (auto& kv : jit_modules) pmx::jit_unload(&kv.second);
    for (auto& kv : jit_modules_big) pmx::jit_unload(&kv.second);
  }
};

// ---- pmx_stream.cpp
// Find or build (plan + upload) the device op stream for this model flavour.
int32_t get_stream(pmx_population* pop, const pmx::CompileKey& key, const pmx::ClassTunables& ct, DeviceStream** out);
// Pick (or fill) the slot holding the sigma tables for `em`.  On return the slot is pinned (host_users) and `stream`
// is ordered after the slot's last use; the caller launches its kernel and then calls release_ll_slot.
int32_t acquire_ll_slot(const pmx_model* model, pmx_population* pop, DeviceStream* ds, const pmx_error_model* em,
                        void* stream, DeviceStream::LLCache** out, bool batch);
void release_ll_slot(pmx_population* pop, DeviceStream::LLCache* slot, void* stream);
// pop->d_subj_obs_off / max_subject_rows, uploaded once per population (the population's device is current)
int32_t resident_obs_off(pmx_population* pop);
// pop->profiles: the host table (pure host work, once per population) / the host table and its device copy (the
// population's device is current)
void host_profiles(pmx_population* pop);
int32_t resident_profiles(pmx_population* pop);
// nullptr, or why the scalars of an exposure call are refused: method, window, threshold, metric bits (both forms)
// (window: {t_start, t_end, threshold} on the host, or null for the whole profile and no threshold)
inline const char* exposure_refusal(int32_t method, const double* window, uint32_t metrics) {
  if (method < PMX_AUC_LINEAR || method > PMX_AUC_LIN_LOG) return "method must be one of PMX_AUC_*";
  if (metrics == 0 || (metrics & ~static_cast<uint32_t>(PMX_EXPO_ALL)) != 0) return "metrics must be a non-empty set of PMX_EXPO_* bits";
  if (window && !(window[0] < window[1])) return "the window needs t_start < t_end (neither NaN)";
  if ((metrics & PMX_EXPO_TIME_ABOVE) && (!window || window[2] != window[2]))
    return "threshold is NaN or not given and PMX_EXPO_TIME_ABOVE is requested";
  return nullptr;
}
struct ExposureWindow {
  double a, b, threshold;
  explicit ExposureWindow(const double* w)
      : a(w ? w[0] : -HUGE_VAL), b(w ? w[1] : HUGE_VAL), threshold(w ? w[2] : 0.0) {}
};

// ---- pmx_launch.cpp
// What the model contributes to the op stream, under this snapshot of the switches, on a population with / without
// infusions: the stream-side half of the walker choice (classed or not, op_kfac rows, propagator slots).
pmx::CompileKey key_for(const pmx_model* m, const pmx::Tunables& tun, bool has_infusions);
// fills model->dev / vol_has_factors from the finished descriptor: the last step of every pmx_model_create*
void finish_model(pmx_model* m);

struct LLRequest {
  const pmx_error_model* em = nullptr;
  double* d_ll = nullptr;
  int64_t ld = 0;
  const int32_t** d_sigma_err = nullptr;  // out (host form): the slot's invalid-sigma counter
};
int32_t enqueue(const pmx_model* model, pmx_population* pop, const double* d_theta, int64_t P, int batch, double* d_pred,
                int64_t ld, uint8_t* d_status, void* stream, const LLRequest* llreq = nullptr, int state_override = -1,
                uint32_t* d_stats = nullptr);

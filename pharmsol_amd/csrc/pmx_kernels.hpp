// pmx_kernels.hpp — host <-> device launch contract (internal to libpmx_hip.so).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "pmx_compile.hpp"
#include "pmx_devtypes.hpp"
#include "pmx_solvers.hpp"

namespace pmx {

// Device mirror of a ClassPlan (pmx_compile.hpp).
struct DevClassPlan {
  const uint32_t* prog_meta;
  const double* prog_dt;
  const double* prog_t0;            // lag models: absolute start of a PROP step / first remaining event time of a RESET step
  const double* prog_t1;            // lag models: absolute end of a PROP step
  const int64_t* cls_prog_off;
  const int32_t* chunk_cls;
  const int32_t* chunk_n;
  const int64_t* chunk_val_off;
  const int32_t* chunk_subj;
  const int64_t* chunk_row;  // [n_chunks*G] first prediction row of each member (0 for padding)
  const double* val;
  const double* prog_rec;           // the programs again, packed for the log-likelihood kernel: [n_prog_steps + 1][2] =
                                    //   {meta (u64 bits), dt} - ONE scalar fetch per step, requested a step ahead
  const uint64_t* chunk_rate_mask;  // [n_chunks] ClassPlan::chunk_rate_mask
  const uint64_t* cls_fast_mask;    // [n_classes] ClassPlan::cls_fast_mask
  const uint32_t* chunk_hdr;        // [n_chunks + 1][16]: everything pmx_analytical_classed_ll needs of a chunk in ONE 64-byte
                                    //   record {n_live | n_steps << 16, program offset, val offset, cobs offset, rate mask (2),
                                    //   class fast mask (2), subject ids (8)} (the last record is padding; null: plan too large)
  const double* dtv;                // loose chunks: each member's own PROP lengths, laid out like val
  const double* facp;               // covariate models: [..][G][n_fac] covariate factors of each member's PROP ...
  const double* faco;               // ... and of the observation fused into the step
  int32_t n_fac;
  int32_t pad_;
  const double* cobs;               // log-likelihood mode: per chunk {[G] sum of the members' constant terms, [G] flags
                                    //   (slot 0: bit k = observation k is plain for every live member),
                                    //   [observation k][2][G] = observed value, weight} (pmx_ll_prepare_chunks)
  const int64_t* chunk_obs_off;     // [n_chunks] offset of the chunk's block in cobs
  const int32_t* generic_subjects;  // subjects the generic GRID kernel still has to walk
  int64_t n_chunks;
  int64_t n_chunks_exact;           // chunks [0, n_chunks_exact): shared step lengths; the rest: loose (pmx_compile.hpp)
  int64_t n_generic;
  int32_t G;
  int32_t zero_status;  // how the analytical GRID kernels own their status bytes (no memset precedes a launch):
                        // 1 = clear with 8-byte stores, then write failures only; 2 = write every pair's byte
};

// Fused per-subject step programs for the lean generic walker (pmx_analytical_steps): what the class plan builds per
// CLASS, built per SUBJECT - every OBS op folded into the step in front of it, one packed 32-byte record per step
// {meta (u64 bits: Kind | Io | ObsAfter | Out | Rung of the op word, pmx_devtypes.hpp), a, b, 0}, one record of padding
// behind the last step (the walker requests step o + 1 while it works on step o).
struct DevSteps {
  const int64_t* subj_step_off;  // [S+1]
  const double* step_rec;        // [(n_steps + 1) * 4]
};

enum LaneMode : int32_t { MODE_GRID = 0, MODE_PAIR = 1 };

// Which kernel serves (part of) a launch, with which template variant and which geometry.  pmx_launch.cpp decides all
// of it (plan_routes) and names it (route_name); the launch_<family> entries of the kernel units only switch on it.
enum RouteFamily : int32_t {
  R_CLASSED,       // pmx_analytical_classed: exact or loose classes
  R_CLASSED_LL,    // pmx_analytical_classed_ll: exact classes of a plain model, log-likelihood
  R_STEPS,         // pmx_analytical_steps: the lean walker over fused step records
  R_DYN3,          // pmx_analytical_dyn3: the matrix-free three-compartment covariate walker
  R_GRID,          // pmx_analytical_grid: the generic walker
  R_PAIR,          // pmx_analytical_pair
  R_ODE,           // pmx_ode_rk4_grid / _pair (mode): built-in diffeq bodies
  R_JIT_ANALYTICAL, R_JIT_ODE, R_JIT_ODE_USER,  // run-time-compiled models (mode)
  R_STATIC_AGRID   // the PMX_DEBUG_STATIC_SO experiment hook
};
struct Route {
  int32_t family;   // RouteFamily
  int32_t mode;     // LaneMode
  bool ll;          // log-likelihood variant
  bool cens;        // ... of a population with censored observations / residual error models (classed kernels' CENS)
  bool loose;       // classed: the loose chunks (per-member step lengths)
  bool lag, dyn;    // lagged input / kernel parameters depend on covariates (re-prepare per PROP)
  bool eig_reuse;   // dyn3: the stream marks segments that repeat the previous built segment's rate constants (EIGR)
  bool leftover;    // walkers behind a classed launch: the subjects of cls.generic_subjects instead of 0..S-1
  int32_t solver;   // ODE: index of the solver's row in kSolvers (pmx_solvers.hpp)
  int64_t n;        // walkers: subjects walked; classed: chunks served
  int32_t s_chunk;  // GRID walkers: subjects walked by one block
  int32_t n_ptiles; // GRID: ceil(P / threads)
  int32_t cpb;      // classed: chunks per block
  uint32_t threads;
  int64_t blocks;
  size_t lds;       // dynamic LDS bytes (kept propagators)
  const char* name; // route_name(*this): what pmx_last_kernel_name reports when this route lends its name
};

struct LaunchArgs {
  DevModel m;
  DevOps ops;
  const double* theta;
  int64_t P, S;
  double* pred;
  int64_t ld;
  uint8_t* status;
  int32_t batch;        // PAIR only: subject s uses theta row s
  int32_t prop_slots;   // DYN GRID: LDS slots for kept propagators (OpStream::prop_cache_used; 0 = none)
  DevClassPlan cls;
  DevSteps steps;       // fused step records of the lean walker (R_STEPS)
  void* stream;
};

// Sigma terms of every observation for one set of error models, computed on the device (AssayErrorModel::sigma,
// error_model.rs:1045-1080; the sigma-only parts of lognormpdf / lognormcdf, distributions.rs:31-103): fills
// obs4[n_obs][4] = {y, -0.5 ln(2 pi) - ln sigma, 1/(2 sigma^2), +-1/(sigma sqrt 2) | 0} and, for a class plan,
// the per-chunk [observation k][value | const | weight][G] blocks.  An invalid sigma (negative, non-finite, or not
// positive on a censored row) poisons that row with NaN and bumps *err.
struct LLPrepareArgs {
  const double* obs_y;        // [n_obs] observed value, NaN = missing
  const int32_t* obs_outeq;   // [n_obs]
  const double* obs_poly;     // [n_obs*4] or nullptr: the observation's own ErrorPoly (c0 NaN = none)
  const int8_t* obs_cens;     // [n_obs] or nullptr
  pmx_error_model em[PMX_MAX_OUT];
  int64_t n_obs;
  double* obs4;
  int32_t* err;
  // classed blocks (n_chunks == 0: none)
  const int64_t* chunk_row;
  const int32_t* chunk_n;
  const int32_t* chunk_nobs;
  const int64_t* chunk_obs_off;
  int64_t n_chunks;
  int32_t G;
  double* cobs;
  // the chunks' programs (flag slot 1 of a chunk's block = the plain-row mask indexed by program STEP)
  const int32_t* chunk_cls;
  const int64_t* cls_prog_off;
  const uint32_t* prog_meta;
  void* stream;
};
hipError_t launch_ll_prepare(const LLPrepareArgs& a);

// *d_flag |= 1 iff any of the n status bytes is non-zero (the host forms' "did any pair fail", without copying the array)
hipError_t launch_status_any(const uint8_t* d_status, int64_t n, int32_t* d_flag, void* stream);

// a linear streaming fill of n_doubles (pmx_measure_write_ceiling)
// (16 bytes per lane: the n_doubles / 2 pairs; the last double of an odd n_doubles is launch_fill_one's)
hipError_t launch_fill_linear(double* d_dst, int64_t n_doubles, double v, void* stream, int shape = 0);  // shape 0..3 (pmx_util.hip)
hipError_t launch_fill_one(double* d_dst, double v, void* stream);  // *d_dst = v, one 8-byte store

// The reductions of a log-likelihood matrix ll[S][ld] (pmx_mixture.hip).
//   lpyl[s] = ln sum_{p: w[p] > 0} w[p] exp(ll[s][p]); a wave owns a row up to kMixtureWaveRowMax columns, a block beyond
constexpr int64_t kMixtureWaveRowMax = 1024;
hipError_t launch_mixture_rows(const double* d_ll, int64_t S, int64_t P, int64_t ld, const double* d_w, double* d_lpyl,
                               void* stream);
//   D[p] = sum_s exp(ll[s][p] - lpyl[s]) - S, in two launches: partial sums of row tiles into d_scratch[n_tiles][n_cand],
//   then the tiles added in order.  A tile is what one wave sums: kDfunctionPasses passes over 64 columns x 1 row, or -
//   n_cand <= 32 - over (1 << cshift) columns x (64 >> cshift) rows.  Pure host arithmetic, shared with
//   pmx_dfunction_scratch_doubles:
constexpr int64_t kDfunctionPasses = 64;
inline int dfunction_cshift(int64_t n_cand) {  // log2 of the columns a wave spans
  int c = 0;
  while (c < 6 && (int64_t{1} << c) < n_cand) ++c;
  return c;
}
inline int64_t dfunction_tiles(int64_t S, int64_t n_cand) {
  const int64_t rows = kDfunctionPasses * (64 >> dfunction_cshift(n_cand));
  return (S + rows - 1) / rows;
}
hipError_t launch_dfunction(const double* d_ll, int64_t S, int64_t n_cand, int64_t ld, const double* d_lpyl,
                            double* d_scratch, double* d_D, void* stream);

// The summaries of a prediction matrix pred[n_obs][ld_pred] over its support points (pmx_posterior.hip).
//   q[s][p] = w[p] exp(ll[s][p] - lpyl[s]) where w[p] > 0, else 0: a wave owns a row of ll, the columns [P, ld_post) of
//   d_post are never written
hipError_t launch_posterior_rows(const double* d_ll, int64_t S, int64_t P, int64_t ld_ll, const double* d_w,
                                 const double* d_lpyl, double* d_post, int64_t ld_post, void* stream);
//   mean[row] = sum_p q pred[row][p] / sum_p q and the lower weighted median of pred[row][.], q the row's subject's
//   posterior (ll, lpyl given) or w itself (both null).  A work item is up to rows_per_item consecutive rows - of one
//   subject in posterior mode - and is owned by a wave up to kSummaryWaveMax columns, by a block of four beyond; the
//   item's q and the row in hand stay in registers up to kSummaryRegisterMax columns, wider rows are re-read.
constexpr int64_t kSummaryWaveMax = 1024, kSummaryRegisterMax = 4096, kSummaryRowsPerItem = 16;
struct SummaryArgs {
  const double* pred;
  int64_t n_obs, P, ld_pred;
  const double* w;
  const double* ll;  // null: population mode
  int64_t ld_ll;
  const double* lpyl;
  const int64_t* subj_obs_off;  // [S + 1], on the device (posterior mode)
  int64_t S, max_subject_rows;
  double* mean;    // [n_obs] or null
  double* median;  // [n_obs] or null
};
hipError_t launch_summary_rows(const SummaryArgs& a, void* stream);

// The exposure metrics of every (profile, support point) of a prediction matrix, and their attainment over the support
// points (pmx_exposure.hip; the arithmetic: include/pmx.h).  The profile table lives on the device: the rows of profile k
// are prof_row[prof_off[k] .. prof_off[k + 1]) with times prof_time[...], in prediction order.
//   A wave owns 64 consecutive columns of one profile, a lane one column; a block is four such waves, consecutive items
//   of the list (profile, column tile) with the column tile fastest.  One plane of `out` per set bit of `metrics`.
struct ExposureArgs {
  const double* pred;
  int64_t P, ld_pred;
  const int64_t* prof_off;  // [n_profiles + 1]
  const int64_t* prof_row;  // [n_obs]
  const double* prof_time;  // [n_obs]
  int64_t n_profiles;
  int32_t method;       // PMX_AUC_*
  double a, b, threshold;
  uint32_t metrics;     // PMX_EXPO_* bits
  double* out;
  int64_t ld_out;
};
hipError_t launch_exposure(const ExposureArgs& a, void* stream);
//   pta[k] and mean[k] of the metric row of profile k under q = w (ll, lpyl null) or the posterior of prof_subject[k]:
//   a wave owns a row up to kAttainWaveMax columns, a block of four beyond
constexpr int64_t kAttainWaveMax = 1024;
struct AttainArgs {
  const double* metric;
  int64_t n_profiles, P, ld_metric;
  const double* target;  // [n_profiles], with pta
  const double* w;
  const double* ll;      // null: population mode
  int64_t ld_ll;
  const double* lpyl;
  const int64_t* prof_subject;  // [n_profiles], on the device (posterior mode)
  double* pta;           // [n_profiles] or null
  double* mean;          // [n_profiles] or null
};
hipError_t launch_attainment(const AttainArgs& a, void* stream);

// One entry per kernel family, at the end of the family's translation unit (pmx_grid.hip, pmx_classed.hip, ...): it
// switches on the model's kernel id and the route's variant flags and enqueues that instantiation.  Policy-free: which
// family, which variant and which geometry is the route's (pmx_launch.cpp plan_routes).
hipError_t launch_classed(const LaunchArgs& a, const Route& r);
hipError_t launch_classed_ll(const LaunchArgs& a, const Route& r);
hipError_t launch_steps(const LaunchArgs& a, const Route& r);
hipError_t launch_dyn3(const LaunchArgs& a, const Route& r);
hipError_t launch_grid(const LaunchArgs& a, const Route& r);
hipError_t launch_pair(const LaunchArgs& a, const Route& r);
hipError_t launch_ode(const LaunchArgs& a, const Route& r);  // (r.mode: grid / pair)

// Enqueue the kernel of one route (a library kernel: not the R_JIT_* / R_STATIC_AGRID families; pmx_launch.cpp).
hipError_t launch_route(const LaunchArgs& a, const Route& r);

// Run-time flags -> template arguments: dispatch(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, ...), so a launch
// is written once for all its variants.  with_kid does the same for the analytical kernel id (an unknown one: error),
// with_solv for the ODE walkers' stepper (SOLV_*).
template <class F>
hipError_t dispatch(F&& f) {
  return f();
}
template <class F, class... Rest>
hipError_t dispatch(F&& f, bool b, Rest... rest) {
  if (b) return dispatch([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
  return dispatch([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
template <int K = 0, class F>
hipError_t with_kid(int32_t kernel, F&& f) {
  if constexpr (K < 12) {
    return kernel == K ? f(std::integral_constant<int, K>{}) : with_kid<K + 1>(kernel, f);
  } else {
    return hipErrorInvalidValue;
  }
}
template <int V = SOLV_AUTO, class F>
hipError_t with_solv(int32_t solv, F&& f) {
  if constexpr (V >= 0) {
    return solv == V ? f(std::integral_constant<int, V>{}) : with_solv<V - 1>(solv, f);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace pmx

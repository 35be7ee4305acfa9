// jit_source_fingerprint — byte-level fingerprint of every text the run-time compilation path generates.
//
// Stand-alone host program: pmx_jit_source.hpp and pmx_jit_source.cpp only (no HIP, no libpmx_hip.so, no Python).  For
// every case of a fixed corpus of named (JitSpec | descriptor) cases it generates the text - a translation unit
// (jit_translation_unit) or a descriptor's closures (ode_descriptor_source, analytical_descriptor_source) - and prints
//
//   <case> <byte length> <64-bit FNV-1a of the text>
//
// tests/golden/jit_source_fingerprints.txt holds that output (tests/test_jit_source_fingerprint.py compares line by
// line, so a mismatch names the case that moved).  The text is the input of the content-keyed code-object cache: a case
// that moves means every user model of that shape is compiled again on every machine.
//
//   jit_source_fingerprint              print the fingerprints
//   jit_source_fingerprint --dump DIR   also write each text to DIR/<case>.hip (diff two dumps to see what moved)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "pmx_jit_source.hpp"

namespace {

// ---- the one place that knows how a JitSpec is filled -----------------------------------------------------------------
pmx::JitSpec make_spec(pmx::JitKind kind, const pmx_model_desc& d, uint32_t fns, bool has_init, int32_t solver, bool big_lists,
                       const char* source) {
  pmx::JitSpec s;
  s.kind = kind;
  s.desc = d;
  s.fns = fns;
  s.has_init = has_init;
  s.solver = solver;
  s.big_lists = big_lists;
  s.source = source;
  return s;
}

// ---- descriptors ------------------------------------------------------------------------------------------------------
pmx_model_desc base(int32_t eq_kind, int32_t kernel, int nstates, int ndrugs, int nout, int nparams) {
  pmx_model_desc d{};
  d.eq_kind = eq_kind;
  d.kernel = kernel;
  d.nstates = nstates;
  d.ndrugs = ndrugs;
  d.nout = nout;
  d.nparams = nparams;
  for (int i = 0; i < PMX_MAX_STATES; ++i) d.init_param[i] = -1;
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) d.lag_param[i] = d.fa_param[i] = d.bolus_dest[i] = d.infusion_dest[i] = -1;
  d.rk4_h_max = 0.125;
  return d;
}
void out(pmx_model_desc* d, int q, int state, int vol_src, int vol_index) { d->out[q] = pmx_out{state, vol_src, vol_index, 0}; }
void bind(pmx_model_desc* d, std::initializer_list<pmx_bind> b) {
  d->n_bind = static_cast<int32_t>(b.size());
  int j = 0;
  for (const pmx_bind& x : b) d->bind[j++] = x;
}
pmx_derived derived(int src_param, std::initializer_list<pmx_factor> f) {
  pmx_derived v{};
  v.src_param = src_param;
  v.n_factors = static_cast<int32_t>(f.size());
  int k = 0;
  for (const pmx_factor& x : f) v.f[k++] = x;
  return v;
}
// the four factor shapes; constants that need all 17 digits (0.1, 1/3) beside one that does not (70)
const pmx_factor kPow{PMX_F_POW, 0, 70.0, 0.75}, kLin{PMX_F_LIN, 1, 0.1, 1.0 / 3.0}, kPowThird{PMX_F_POW, 1, 1.0 / 3.0, -0.1};
void four_derived(pmx_model_desc* d) {
  d->n_covariates = 2;
  d->n_derived = 4;
  d->derived[0] = derived(0, {});
  d->derived[1] = derived(1, {kPow});
  d->derived[2] = derived(2, {kLin});
  d->derived[3] = derived(1, {kPowThird, kLin});
}

// ---- fingerprint ------------------------------------------------------------------------------------------------------
const char* g_dump = nullptr;
int g_failures = 0;
void emit(const std::string& name, const std::string& text) {
  uint64_t h = 0xcbf29ce484222325ULL;
  for (unsigned char c : text) h = (h ^ c) * 0x100000001b3ULL;
  std::printf("%s %zu %016" PRIx64 "\n", name.c_str(), text.size(), h);
  if (!g_dump) return;
  const std::string path = std::string(g_dump) + "/" + name + ".hip";
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size()) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    ++g_failures;
  }
  if (f) std::fclose(f);
}

const char* const kAnSource = "PMX_DEVICE void pmx_route_lag(double t, const double* x, const double* p, const double* cov,\n"
                              "    const double* rateiv, const double* derived, double* lag) { lag[0] = p[2]; }\n";
const char* const kOdeSource = "PMX_DEVICE void pmx_dynamics(double t, const double* x, const double* p, const double* cov,\n"
                               "    const double* rateiv, const double* derived, double* dx) { dx[0] = -p[0] * x[0] + rateiv[0]; }\n"
                               "PMX_DEVICE void pmx_outputs(double t, const double* x, const double* p, const double* cov,\n"
                               "    const double* rateiv, const double* derived, double* y) { y[0] = x[0] / p[1]; }";

// ---- the corpus -------------------------------------------------------------------------------------------------------
void analytical_units() {
  const auto unit = [](const char* name, const pmx_model_desc& d, uint32_t fns, bool big_lists = false, const char* src = kAnSource) {
    emit(name, pmx::jit_translation_unit(make_spec(pmx::JIT_ANALYTICAL, d, fns, false, PMX_SOLVER_RK4, big_lists, src)));
  };
  {  // a built-in structure, identity projection, no closure at all: every closure body empty or from the descriptor
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_TWO_COMPARTMENTS, 2, 1, 1, 4);
    out(&d, 0, 0, PMX_SRC_PRIMARY, 3);
    unit("an_builtin_plain", d, 0, false, "");
    unit("an_builtin_plain_big", d, 0, true, "");
  }
  {  // n_bind > 0, all primary; an output without a volume
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_ONE_COMPARTMENT_CL, 1, 1, 1, 3);
    bind(&d, {{PMX_SRC_PRIMARY, 2}, {PMX_SRC_PRIMARY, 0}});
    out(&d, 0, 0, PMX_SRC_NONE, 0);
    unit("an_bind_primary", d, PMX_FN_ROUTE_LAG);
  }
  {  // a bind on a derived value (no static coefficients), derive closure, derived volume, absolute covariate time
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_ONE_COMPARTMENT_CL_WITH_ABSORPTION, 2, 1, 1, 4);
    d.n_covariates = 2;
    d.n_derived = 2;
    d.cov_time_mode = PMX_COV_TIME_SEGMENT_END_ABS;
    bind(&d, {{PMX_SRC_PRIMARY, 0}, {PMX_SRC_DERIVED, 0}, {PMX_SRC_DERIVED, 1}});
    out(&d, 0, 1, PMX_SRC_DERIVED, 1);
    unit("an_bind_derived_abs", d, PMX_FN_DERIVE);
    d.cov_time_mode = PMX_COV_TIME_SEGMENT_DT;
    unit("an_bind_derived_dt", d, PMX_FN_DERIVE | PMX_FN_ROUTE_BIOAVAILABILITY, true);
  }
  {  // the user's own propagator; pm indexing asked for and ignored
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_CUSTOM, 3, 2, 2, 5);
    d.pmetrics_indexing = 1;
    unit("an_custom_eq", d, PMX_FN_EQ | PMX_FN_OUTPUTS);
    d.pmetrics_indexing = 0;
    d.n_derived = 1;
    unit("an_custom_all_closures", d,
         PMX_FN_EQ | PMX_FN_OUTPUTS | PMX_FN_INIT | PMX_FN_DERIVE | PMX_FN_ROUTE_LAG | PMX_FN_ROUTE_BIOAVAILABILITY | PMX_FN_SEQ_EQ);
  }
  {  // lag / fa / init / outputs from the descriptor: three inputs, gaps between them; none, primary, derived volume; pm indexing
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_TWO_COMPARTMENTS_WITH_ABSORPTION, 3, 3, 3, 8);
    d.pmetrics_indexing = 1;
    d.n_derived = 2;
    d.lag_param[0] = 4, d.lag_param[2] = 5;
    d.fa_param[1] = 6;
    d.init_param[1] = 7, d.init_param[2] = 0;
    out(&d, 0, 1, PMX_SRC_NONE, 0);
    out(&d, 1, 1, PMX_SRC_PRIMARY, 3);
    out(&d, 2, 2, PMX_SRC_DERIVED, 1);
    unit("an_desc_closures_pm", d, PMX_FN_DERIVE);
    unit("an_desc_closures_seq", d, PMX_FN_DERIVE | PMX_FN_SEQ_EQ | PMX_FN_INIT);
  }
  {  // ndrugs 0 counts as one input; a lag parameter on an input the model does not have sets HAS_LAG and writes no line
    pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_ONE_COMPARTMENT, 1, 0, 1, 2);
    d.lag_param[3] = 1;
    d.fa_param[0] = 1;
    out(&d, 0, 0, PMX_SRC_NONE, 0);
    unit("an_no_drugs", d, 0);
  }
}

void user_ode_units() {
  const auto unit = [](const std::string& name, const pmx_model_desc& d, uint32_t fns, int32_t solver, bool big_lists = false) {
    emit(name, pmx::jit_translation_unit(make_spec(pmx::JIT_ODE_USER, d, fns, false, solver, big_lists, kOdeSource)));
  };
  const uint32_t body = PMX_FN_DYNAMICS | PMX_FN_OUTPUTS;
  pmx_model_desc plain = base(PMX_EQ_ODE, PMX_ODE_CUSTOM, 1, 1, 1, 3);
  for (const pmx::SolverRow& r : pmx::kSolvers)  // no derive, no init, lag as closure
    unit(std::string("uode_lag_closure_") + r.name, plain, body | PMX_FN_ROUTE_LAG, r.id);
  unit("uode_fa_closure_big", plain, body | PMX_FN_ROUTE_BIOAVAILABILITY, PMX_SOLVER_RK4, true);
  {  // every closure, the bolus form of the dynamics, three derived values
    pmx_model_desc d = base(PMX_EQ_ODE, PMX_ODE_CUSTOM, 2, 2, 2, 4);
    d.n_covariates = 1;
    d.n_derived = 3;
    unit("uode_all_closures_bolus", d,
         PMX_FN_DYNAMICS_BOLUS | PMX_FN_OUTPUTS | PMX_FN_INIT | PMX_FN_DERIVE | PMX_FN_ROUTE_LAG | PMX_FN_ROUTE_BIOAVAILABILITY,
         PMX_SOLVER_DOPRI5);
    unit("uode_bolus_init_no_derive", d, PMX_FN_DYNAMICS_BOLUS | PMX_FN_OUTPUTS | PMX_FN_INIT, PMX_SOLVER_AUTO, true);
  }
  {  // derive with n_derived 0 (one slot); lag / fa / init from the descriptor; ndrugs 0
    pmx_model_desc d = base(PMX_EQ_ODE, PMX_ODE_CUSTOM, 3, 0, 1, 6);
    d.lag_param[0] = 3;
    d.fa_param[0] = 4;
    d.init_param[0] = 5, d.init_param[2] = 1;
    unit("uode_desc_closures_derive", d, body | PMX_FN_DERIVE, PMX_SOLVER_ROS2);
    d.ndrugs = 3;
    d.lag_param[2] = 2;
    d.fa_param[1] = 0, d.fa_param[5] = 1;
    unit("uode_desc_closures", d, body, PMX_SOLVER_RK4_CHECKED);
  }
}

void state_machine_units() {
  for (const pmx::SolverRow& r : pmx::kSolvers) {
    pmx_model_desc d = base(PMX_EQ_ODE, PMX_ODE_CUSTOM, 1, 0, 1, 2);
    emit(std::string("sm_") + r.name, pmx::jit_translation_unit(make_spec(pmx::JIT_ODE, d, 0, false, r.id, false, kOdeSource)));
    d = base(PMX_EQ_ODE, PMX_ODE_CUSTOM, 4, 3, 2, 7);
    d.n_covariates = 2;
    emit(std::string("sm_init_3drugs_") + r.name, pmx::jit_translation_unit(make_spec(pmx::JIT_ODE, d, 0, true, r.id, false, kOdeSource)));
  }
}

void ode_descriptor_sources() {
  static const int kNP[PMX_ODE_MODEL_COUNT] = {1, 2, 3, 4, 5, 6, 3}, kNS[PMX_ODE_MODEL_COUNT] = {1, 2, 2, 3, 3, 4, 1};
  for (int k = 0; k < PMX_ODE_MODEL_COUNT; ++k) {
    const std::string name = "odesc_k" + std::to_string(k);
    // identity projection, no derived value, default infusion destinations, a primary volume
    pmx_model_desc d = base(PMX_EQ_ODE, k, kNS[k], k % 3, 1, kNP[k] + 1);
    out(&d, 0, kNS[k] - 1, PMX_SRC_PRIMARY, kNP[k]);
    emit(name + "_plain", pmx::ode_descriptor_source(d));
    // every kernel parameter bound, odd ones to derived values; the four factor shapes; routed infusions; init parameters
    d = base(PMX_EQ_ODE, k, kNS[k], 3, 3, kNP[k] + 2);
    four_derived(&d);
    d.n_bind = kNP[k];
    for (int j = 0; j < kNP[k]; ++j) d.bind[j] = (j & 1) ? pmx_bind{PMX_SRC_DERIVED, j % 4} : pmx_bind{PMX_SRC_PRIMARY, kNP[k] - j};
    d.infusion_dest[0] = kNS[k] - 1, d.infusion_dest[2] = 0;
    d.init_param[0] = kNP[k] + 1;
    if (kNS[k] > 2) d.init_param[2] = 1;
    out(&d, 0, 0, PMX_SRC_NONE, 0);
    out(&d, 1, kNS[k] - 1, PMX_SRC_PRIMARY, 1);
    out(&d, 2, 0, PMX_SRC_DERIVED, 3);
    emit(name + "_derived", pmx::ode_descriptor_source(d));
  }
}

void analytical_descriptor_sources() {
  pmx_model_desc d = base(PMX_EQ_ANALYTICAL, PMX_K_ONE_COMPARTMENT, 1, 1, 1, 3);
  emit("adesc_none", pmx::analytical_descriptor_source(d));
  four_derived(&d);
  emit("adesc_four_shapes", pmx::analytical_descriptor_source(d));
  // two derived values in a row with a floating-point constant each: the second prints in the form the first one set
  d.n_derived = 2;
  d.derived[0] = derived(2, {kLin, kPow});
  d.derived[1] = derived(0, {kPowThird});
  emit("adesc_two_in_a_row", pmx::analytical_descriptor_source(d));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--dump") == 0) {
    g_dump = argv[2];
  } else if (argc != 1) {
    std::fprintf(stderr, "usage: %s [--dump DIR]\n", argv[0]);
    return 2;
  }
  analytical_units();
  user_ode_units();
  state_machine_units();
  ode_descriptor_sources();
  analytical_descriptor_sources();
  return g_failures ? 1 : 0;
}

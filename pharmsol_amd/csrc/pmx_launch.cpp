// pmx_launch.cpp — which kernel serves a call: the compile key (the stream-side half of the choice), the route(s) of
// a launch with their geometry and names, and enqueue, which binds the arguments and launches them.
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <set>

#include "pmx_internal.hpp"
#include "pmx_structures.hpp"  // kernel_structure(), kernel_nparams(), Structure<ST>::Prop

namespace pmx {

void Tunables::load() {
  auto flag = [](const char* n) {
    const char* e = std::getenv(n);
    return e && e[0] && e[0] != '0';
  };
  auto num = [](const char* n) {
    const char* e = std::getenv(n);
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : 0;
  };
  auto tri = [](const char* n) {
    const char* e = std::getenv(n);
    return e ? ((e[0] && e[0] != '0') ? 1 : 0) : -1;
  };
  disable_ladder = flag("PMX_DISABLE_LADDER");
  disable_classing = flag("PMX_DISABLE_CLASSING");
  disable_steps = std::getenv("PMX_DISABLE_STEPS") != nullptr;
  disable_dyn3 = std::getenv("PMX_DISABLE_DYN3") != nullptr;
  ll_old = flag("PMX_TUNE_LL_OLD");
  steps_per_trip = num("PMX_TUNE_STEPS_PER_TRIP");
  grid_min_p = num("PMX_TUNE_GRID_MIN_P");
  cls.min_class = num("PMX_TUNE_MIN_CLASS");
  cpb = num("PMX_TUNE_CPB");
  {
    const char* e = std::getenv("PMX_TUNE_PROP_SLOTS");
    prop_slots = e ? std::atoi(e) : -1;
  }
  dyn_tile = num("PMX_TUNE_DYN_TILE");
  cls.spread = tri("PMX_TUNE_SPREAD");
  cls.loose = tri("PMX_TUNE_LOOSE");
  jit_cache = tri("PMX_JIT_CACHE") != 0;
  jit_cache_entries = num("PMX_JIT_CACHE_ENTRIES") > 0 ? num("PMX_JIT_CACHE_ENTRIES") : 64;  // (64: a policy choice, not a measurement)
  {
    static std::set<std::string> dirs;  // (load() runs under g_tun_mu)
    const char* e = std::getenv("PMX_JIT_CACHE_DIR");
    jit_cache_dir = (e && e[0]) ? dirs.insert(e).first->c_str() : nullptr;
  }
}

namespace {
std::mutex g_tun_mu;
Tunables g_tun;
bool g_tun_loaded = false;
}  // namespace
Tunables tunables() {
  std::lock_guard<std::mutex> lock(g_tun_mu);
  if (!g_tun_loaded) {
    g_tun.load();
    g_tun_loaded = true;
  }
  return g_tun;
}
void reload_tunables() {
  std::lock_guard<std::mutex> lock(g_tun_mu);
  g_tun.load();
  g_tun_loaded = true;
}

}  // namespace pmx

using pmx::Route;
using pmx::Tunables;

namespace {

// bytes of a kept propagator / doubles of a kept matrix-free segment, per structure (S_ONE .. S_THREE_ABS)
constexpr size_t kPropBytes[6] = {sizeof(pmx::Structure<pmx::S_ONE>::Prop),     sizeof(pmx::Structure<pmx::S_ONE_ABS>::Prop),
                                  sizeof(pmx::Structure<pmx::S_TWO>::Prop),     sizeof(pmx::Structure<pmx::S_TWO_ABS>::Prop),
                                  sizeof(pmx::Structure<pmx::S_THREE>::Prop),   sizeof(pmx::Structure<pmx::S_THREE_ABS>::Prop)};
constexpr size_t kDirect0Doubles[6] = {0, 0, 0, 0, pmx::kHasDirect0<pmx::S_THREE> ? pmx::Structure<pmx::S_THREE>::ND0 : 0,
                                       pmx::kHasDirect0<pmx::S_THREE_ABS> ? pmx::Structure<pmx::S_THREE_ABS>::ND0 : 0};

}  // namespace

pmx::CompileKey key_for(const pmx_model* m, const Tunables& tun, bool has_infusions) {
  pmx::CompileKey k;
  k.eq_kind = m->d.eq_kind;
  if (m->d.eq_kind == PMX_EQ_ANALYTICAL && m->custom) {
    // user closures (pmx_analytical.hpp): covariates are looked up on the device, so the stream carries no factors;
    // absolute times on every PROP, solve marks for seq_eq, every input's rate for a user propagator, and - when the
    // model has any lag closure - ALL boluses leave the stream into one list per occasion that each lane sorts itself
    k.cov_time_mode = PMX_COV_TIME_SEGMENT_DT;  // (unused: no host-side covariate evaluation)
    k.rk4_h_max = 0.0;
    k.rate_input = (m->d.pmetrics_indexing && !m->user_eq) ? 1 : 0;  // (pm_* wrappers read rateiv[1]: analytical/mod.rs:86-88)
    k.full_rates = m->user_eq;
    k.n_rate = m->user_eq ? (m->d.ndrugs > 0 ? m->d.ndrugs : 1) : 1;
    k.want_times = true;
    k.solve_marks = true;
    k.user_cov = true;
    if (m->user_lag) {
      k.lag_merge = true;
      for (int i = 0; i < m->d.ndrugs && i < PMX_MAX_INPUTS; ++i) k.lag_mask |= (1u << i);
    }
  } else if (m->d.eq_kind == PMX_EQ_ANALYTICAL) {
    k.cov_time_mode = m->d.cov_time_mode;
    k.rk4_h_max = 0.0;
    k.n_rate = 1;
    k.rate_input = m->d.pmetrics_indexing ? 1 : 0;
    // classed fast path: theta-only coefficients, no covariates, plain indexing
    for (int i = 0; i < PMX_MAX_INPUTS; ++i)
      if (m->d.lag_param[i] >= 0) k.lag_mask |= (1u << i);
    // (bioavailability does not stop classing: the amounts in the plan are the recorded ones, each lane scales them)
    k.ladder = !m->dyn && k.lag_mask == 0 && !tun.disable_ladder;  // (switch: fresh exp() on every step, A/B and parity checks)
    k.n_derived = m->d.n_derived;
    std::memcpy(k.derived, m->d.derived, sizeof(k.derived));
    const bool disabled = tun.disable_classing;
    bool reads_pad = false;  // pm_ indexing: an output on model state 0 reads the wrapper's pad slot (generic walker only)
    if (m->d.pmetrics_indexing)
      for (int o = 0; o < m->d.nout && o < PMX_MAX_OUT; ++o)
        if (m->d.out[o].state == 0) reads_pad = true;
    // (one lagged input is classed too: in an exact class the bolus times are shared, so a lane's split points and the
    // propagator of every sub-interval serve all G members)
    const bool lag_ok = (k.lag_mask & (k.lag_mask - 1u)) == 0u;
    // (covariate-derived constants are classed by program shape alone, each member with its own factor rows)
    const bool plain = !m->dyn && m->d.n_covariates == 0;
    // ... where it pays: the one- and two-state structures (1-cpt + absorption 3.41 -> 2.87 ms on the C5 design); from
    // three states up the rebuild is so dominated by its own arithmetic that the batch gains nothing (C5: 19.4 -> 19.9 ms)
    const int st = pmx::kernel_structure(m->d.kernel);
    const bool dyn_ok = m->dyn && !m->d.pmetrics_indexing && k.lag_mask == 0 &&
                        (st == pmx::S_ONE || st == pmx::S_ONE_ABS || st == pmx::S_TWO);
    if (!disabled && !reads_pad && lag_ok && (plain || dyn_ok)) {
      k.class_g = (st == pmx::S_ONE || st == pmx::S_ONE_ABS || st == pmx::S_TWO) ? 8 : 4;  // == ClassBatch<KID>::G
    }
    // covariate models that take the generic walker: equal (length, factors) PROPs of an occasion share a propagator
    if (m->dyn && k.lag_mask == 0 && k.class_g == 0 && (st == pmx::S_THREE || st == pmx::S_THREE_ABS) && !m->d.pmetrics_indexing) {
      k.kfac_n = pmx::kernel_nparams(m->d.kernel);  // (the matrix-free walker, pmx_analytical_dyn3)
      for (int j = 0; j < k.kfac_n && j < 8; ++j)
        k.kfac_map[j] = (m->d.n_bind > 0 && m->d.bind[j].src == PMX_SRC_DERIVED) ? static_cast<int8_t>(m->d.bind[j].index) : int8_t(-1);
    }
    if (m->dyn && k.lag_mask == 0 && k.class_g == 0) {
      k.prop_cache_slots = tun.prop_slots >= 0 ? (tun.prop_slots > 3 ? 3 : tun.prop_slots) : 1;
      // the kept propagators live in LDS, [slot][component][256 lanes]: stay inside the 64 KB a block may take without an
      // opt-in attribute (the stream's cache codes are written for THIS number of slots, so it is fixed here)
      const int per_slot = static_cast<int>(kPropBytes[st]) * 256;
      while (k.prop_cache_slots > 0 && k.prop_cache_slots * per_slot > (64 << 10)) --k.prop_cache_slots;
      // a population without infusions takes the matrix-free walker, whose kept segment is 6-7 numbers per lane: two slots
      // fit where the matrix form held one (C5: 8 rebuilds per subject instead of 9)
      if (k.kfac_n > 0 && k.prop_cache_slots == 1 && tun.prop_slots < 0 && !tun.disable_dyn3 && !has_infusions) k.prop_cache_slots = 2;
    }  // (one slot: a second costs more occupancy
    // than its extra reuse returns - C5: 1 slot 16.8 ms, 2 slots 19.4 ms, none 20.2 ms; tools/c5 notes in DESIGN.md)
  } else if (m->user_ode) {
    // ODE with user lag / fa / derive closures (pmx_ode_user.hpp): covariates are looked up on the device, every PROP
    // carries its absolute [t0, t1), every input's rate rides along, and - when the model has any lag closure - ALL
    // boluses leave the stream into one list per occasion that each lane sorts itself
    k.cov_time_mode = PMX_COV_TIME_SEGMENT_END_ABS;
    k.rk4_h_max = m->d.rk4_h_max;
    k.n_rate = m->d.ndrugs > 0 ? m->d.ndrugs : 1;
    k.rate_input = 0;
    k.want_times = true;
    k.user_cov = true;
    if (m->user_lag) {
      k.lag_merge = true;
      for (int i = 0; i < m->d.ndrugs && i < PMX_MAX_INPUTS; ++i) k.lag_mask |= (1u << i);
    }
  } else {
    k.cov_time_mode = PMX_COV_TIME_SEGMENT_END_ABS;
    k.rk4_h_max = m->d.rk4_h_max;
    k.n_rate = m->d.ndrugs > 0 ? m->d.ndrugs : 1;
    k.rate_input = 0;
    for (int i = 0; i < PMX_MAX_INPUTS; ++i)
      if (m->d.lag_param[i] >= 0) k.lag_mask |= (1u << i);
    // absolute piece times: a user body may be non-autonomous; the adaptive solvers step on [t0, t1] themselves
    k.want_times = m->custom || pmx::solver_row(m->d.ode_solver)->want_times;
  }
  return k;
}

void finish_model(pmx_model* model) {
  const pmx_model_desc& d = model->d;
  pmx::DevModel& m = model->dev;
  m = pmx::DevModel{};
  m.eq_kind = d.eq_kind;
  m.kernel = d.kernel;
  m.nparams = d.nparams;
  m.n_cov = d.n_covariates;
  m.n_derived = d.n_derived;
  m.n_bind = d.n_bind;
  m.nout = d.nout;
  m.pm = d.pmetrics_indexing ? 1 : 0;
  m.has_init = model->has_init ? 1 : 0;
  m.rk4_h_max = d.rk4_h_max;
  m.ode_rtol = d.ode_rtol;
  m.ode_atol = d.ode_atol;
  m.ode_stiff = (d.eq_kind == PMX_EQ_ODE && pmx::solver_row(d.ode_solver)->stiff) ? 1 : 0;
  std::memcpy(m.derived, d.derived, sizeof(d.derived));
  std::memcpy(m.bind, d.bind, sizeof(d.bind));
  std::memcpy(m.out, d.out, sizeof(d.out));
  m.state_override = -1;  // (enqueue patches a copy for pmx_predict_state_device)
  for (int o = 0; o < PMX_MAX_OUT; ++o) {
    m.out_vol_theta[o] = -1;
    if (m.out[o].vol_src == PMX_SRC_PRIMARY) m.out_vol_theta[o] = m.out[o].vol_index;
    if (m.out[o].vol_src == PMX_SRC_DERIVED && m.out[o].vol_index >= 0 && m.out[o].vol_index < PMX_MAX_DERIVED)
      m.out_vol_theta[o] = d.derived[m.out[o].vol_index].src_param;
  }
  std::memcpy(m.init_param, d.init_param, sizeof(d.init_param));
  std::memcpy(m.bolus_dest, d.bolus_dest, sizeof(d.bolus_dest));
  std::memcpy(m.infusion_dest, d.infusion_dest, sizeof(d.infusion_dest));
  std::memcpy(m.fa_param, d.fa_param, sizeof(d.fa_param));
  for (int i = 0; i < PMX_MAX_INPUTS; ++i) {
    if (d.fa_param[i] >= 0) m.has_fa = 1;
    if (d.lag_param[i] >= 0 && m.n_lag_slots < pmx::kMaxLagSlots && !model->user_ode) {
      m.lag_input[m.n_lag_slots] = i;
      m.lag_param[m.n_lag_slots] = d.lag_param[i];
      m.lag_dest[m.n_lag_slots] = (d.eq_kind == PMX_EQ_ODE && d.bolus_dest[i] >= 0) ? d.bolus_dest[i] : i;
      m.n_lag_slots++;
    }
  }
  model->vol_has_factors = false;
  for (int o = 0; o < d.nout && o < PMX_MAX_OUT; ++o)
    if (d.out[o].vol_src == PMX_SRC_DERIVED && d.out[o].vol_index >= 0 && d.out[o].vol_index < PMX_MAX_DERIVED &&
        d.derived[d.out[o].vol_index].n_factors > 0)
      model->vol_has_factors = true;
}

namespace {

// (experiment hook, tools/experiments/user_static: PMX_DEBUG_STATIC_SO names a shared object holding the SAME translation
// unit compiled ahead of time by hipcc, with a launcher for its GRID prediction entry point)
typedef int (*static_launch_t)(const void*, const void*, const double*, int64_t, int64_t, int32_t, int32_t, double*, int64_t,
                               uint8_t*, uint32_t, uint32_t, void*);
static_launch_t static_launcher() {
  static static_launch_t s_static = []() -> static_launch_t {
    const char* so = std::getenv("PMX_DEBUG_STATIC_SO");
    if (!so) return nullptr;
    void* h = dlopen(so, RTLD_NOW | RTLD_LOCAL);
    return h ? reinterpret_cast<static_launch_t>(dlsym(h, "pmx_static_launch")) : nullptr;
  }();
  return s_static;
}

// THE name of a route: every string pmx_last_kernel_name can return is written (the ODE ones: put together) here.
const char* route_name(const Route& r) {
  // the ODE names, built once from the solver table's fragments: pmx_ode_rk4_grid, pmx_jit_ode_auto_pair<lag>, ...
  struct OdeNames {
    std::string s[3][pmx::kNumSolvers][2][2];  // [built-in | run-time-compiled | ... with user closures][row][pair][lag]
    OdeNames() {
      static const char* const kPrefix[3] = {"pmx_ode_", "pmx_jit_ode_", "pmx_jit_ode_user_"};
      for (int f = 0; f < 3; ++f)
        for (int i = 0; i < pmx::kNumSolvers; ++i)
          for (int pair = 0; pair < 2; ++pair)
            for (int lag = 0; lag < 2; ++lag)
              s[f][i][pair][lag] = std::string(kPrefix[f]) + pmx::kSolvers[i].name + (pair ? "_pair" : "_grid") + (lag ? "<lag>" : "");
    }
  };
  static const OdeNames kOde;
  const int pair = r.mode == pmx::MODE_PAIR ? 1 : 0;
  switch (r.family) {
    case pmx::R_CLASSED:
      if (r.loose && r.dyn) return r.ll ? "pmx_analytical_classed<ll,dyn>" : "pmx_analytical_classed<dyn>";
      if (r.loose) return r.ll ? "pmx_analytical_classed<ll,loose>" : "pmx_analytical_classed<loose>";
      if (r.lag) return r.ll ? "pmx_analytical_classed<ll,lag>" : "pmx_analytical_classed<lag>";
      return r.ll ? "pmx_analytical_classed<ll>" : "pmx_analytical_classed";
    case pmx::R_CLASSED_LL: return "pmx_analytical_classed_ll";
    case pmx::R_STEPS: return "pmx_analytical_steps";
    case pmx::R_DYN3: return "pmx_analytical_dyn3";
    case pmx::R_GRID: return r.dyn ? "pmx_analytical_grid<dyn>" : (r.lag ? "pmx_analytical_grid<lag>" : "pmx_analytical_grid");
    case pmx::R_PAIR: return r.dyn ? "pmx_analytical_pair<dyn>" : (r.lag ? "pmx_analytical_pair<lag>" : "pmx_analytical_pair");
    case pmx::R_ODE: return kOde.s[0][r.solver][pair][r.lag ? 1 : 0].c_str();
    case pmx::R_JIT_ODE: return kOde.s[1][r.solver][pair][r.lag ? 1 : 0].c_str();
    case pmx::R_JIT_ODE_USER: return kOde.s[2][r.solver][pair][0].c_str();
    case pmx::R_JIT_ANALYTICAL: return pair ? "pmx_jit_analytical_pair" : "pmx_jit_analytical_grid";
    case pmx::R_STATIC_AGRID: return "pmx_static_agrid";
  }
  return "";
}

// The kernels of one launch, in launch order: exact classes, loose classes, then the walker of the subjects no class
// holds - or the one kernel that serves everybody.
struct Routes {
  int32_t mode = pmx::MODE_PAIR;  // LaneMode of the whole launch
  Route r[3] = {};
  int n = 0;
  // What pmx_last_kernel_name reports: the first kernel launched lends its name - except that the loose launch of a
  // covariate model always does (its exact classes, if any, are the odd ones out).
  const char* name() const {
    const char* s = n > 0 ? r[0].name : "";
    for (int i = 0; i < n; ++i)
      if (r[i].family == pmx::R_CLASSED && r[i].loose && r[i].dyn) s = r[i].name;
    return s;
  }
  void add(Route x) {
    x.name = route_name(x);
    r[n++] = x;
  }
};

// GRID launches: a support grid smaller than one 256-lane tile runs with just the waves it needs (whole waves of
// lanes beyond n_support would otherwise walk every subject for nothing: P = 64 wasted 3 of 4 waves).
inline uint32_t grid_threads(int64_t P) {
  return P <= 64 ? 64u : (P <= 128 ? 128u : 256u);  // (192-thread blocks measured slower than 256)
}

// What a launch is asked for, besides the model and the stream.
struct Call {
  int64_t S, P;  // P = 1 for batch calls
  bool batch, ll, cens;
  int64_t ll_ld;
  bool raw_state;  // pmx_predict_state_device: outputs are raw state amounts (no volumes)
};

// the classed kernels: enough blocks to fill the chip several times over, few enough that lane_setup stays amortised
// (chunks are taken in grid-stride order; one chunk per block up to 32k blocks measured best: tools/experiments/cpb_on_one_allocation.py)
// (the log-likelihood variant writes almost nothing: it prefers fewer, longer blocks that amortise the lane setup)
// (the loose launch is FP64-bound too and behaves the same: 4 chunks per block 1.83 ms, one 1.88 ms, eight 1.84 ms
// on jittered C3, profiles/r02/loose_chunks_per_block.txt)
Route classed_route(Route r, int64_t n_chunks, const Tunables& tun) {
  int64_t cpb = (n_chunks * r.n_ptiles) / ((r.ll || r.loose) ? 8192 : 32768);
  if (cpb < 1) cpb = 1;
  if (cpb > (r.loose && !r.ll ? 4 : 8)) cpb = r.loose && !r.ll ? 4 : 8;
  if (tun.cpb > 0) cpb = tun.cpb;  // tuning experiments (PMX_TUNE_CPB)
  r.n = n_chunks;
  r.cpb = static_cast<int32_t>(cpb);
  r.blocks = (((n_chunks + cpb - 1) / cpb + 7) / 8 * 8) * r.n_ptiles;  // whole XCD groups
  return r;
}

// the analytical GRID walker of `n` subjects: lean steps, matrix-free dyn3 or the generic one
Route walker_route(Route r, const pmx_model& model, const StreamFacts& f, const Call& c, int64_t n, const Tunables& tun) {
  const int st = pmx::kernel_structure(model.d.kernel);
  r.n = n;
  if (r.leftover) {
    const int64_t ch = (n * r.n_ptiles) / 8192;
    r.s_chunk = static_cast<int32_t>(ch < 1 ? 1 : (ch > 64 ? 64 : ch));
  }
  // tile = support points per block.  With kept propagators (DYN) the LDS cache is sized per lane, so the tile also
  // sets the occupancy: PMX_TUNE_DYN_TILE (64 / 128 / 256; 0 = the default tile; 64 and 256 measured the same with one slot)
  if (r.dyn && f.prop_slots > 0) {
    if (tun.dyn_tile > 0 && static_cast<uint32_t>(tun.dyn_tile) < r.threads) r.threads = static_cast<uint32_t>(tun.dyn_tile);
    r.n_ptiles = static_cast<int32_t>((c.P + r.threads - 1) / r.threads);
    r.lds = static_cast<size_t>(f.prop_slots) * kPropBytes[st] * r.threads;
  }
  r.blocks = ((n + r.s_chunk - 1) / r.s_chunk) * r.n_ptiles;
  // the lean walker serves the plain models: rate constants and volumes fixed per lane, no lag, no pm_ pad slot
  const bool plain = !r.dyn && !r.lag && !model.d.pmetrics_indexing && !tun.disable_steps &&
                     (c.raw_state || !model.vol_has_factors);
  // three-compartment covariate model, no infusion anywhere: the matrix-free walker
  const bool no_rates = f.no_rates && f.has_kfac && !tun.disable_dyn3;
  r.family = pmx::R_GRID;
  if (plain && f.has_steps) {
    r.family = pmx::R_STEPS;
  } else if (r.dyn && !r.lag && kDirect0Doubles[st] > 0 && no_rates && !model.d.pmetrics_indexing) {
    r.family = pmx::R_DYN3;
    r.eig_reuse = f.eig_reuse;
    r.lds = f.prop_slots > 0 ? static_cast<size_t>(f.prop_slots) * kDirect0Doubles[st] * sizeof(double) * r.threads : 0;
  }
  return r;
}

// THE walker choice of a launch: family, variant, mode and geometry of every kernel it takes.
Routes plan_routes(const pmx_model& model, const StreamFacts& f, const Call& c, const Tunables& tun) {
  const pmx_model_desc& d = model.d;
  const bool analytical = d.eq_kind == PMX_EQ_ANALYTICAL;
  Routes out;
  // GRID (lane = support point, wave-uniform op stream) vs PAIR (lane = pair, divergent streams): measured crossovers
  // (tools/experiments/pairgrid_sweep.sh) are 8 support points when the classed kernel serves most subjects, ~48 when every
  // subject goes through the generic walker (a GRID wave with few live lanes still pays the whole walk); ODE: 32.
  int64_t grid_min_p = 32;
  if (analytical) grid_min_p = (f.n_chunks > 0 && 2 * f.n_classed_subjects >= c.S) ? 8 : 48;
  if (tun.grid_min_p > 0) grid_min_p = tun.grid_min_p;  // tuning experiments
  Route r{};
  r.ll = c.ll;
  r.cens = c.ll && c.cens;
  if (!c.batch && c.P >= grid_min_p) {
    r.mode = pmx::MODE_GRID;
    r.threads = grid_threads(c.P);
    r.n_ptiles = static_cast<int32_t>((c.P + 255) / 256);
    // enough blocks to fill 256 CUs several times over, few enough that the per-block
    // rate-constant setup stays amortised
    int64_t chunk = (c.S * r.n_ptiles) / 8192;
    if (chunk < 1) chunk = 1;
    if (chunk > 64) chunk = 64;
    r.s_chunk = static_cast<int32_t>(chunk);
    r.blocks = ((c.S + r.s_chunk - 1) / r.s_chunk) * r.n_ptiles;
  } else {
    r.mode = pmx::MODE_PAIR;
    r.threads = 256;
    r.n_ptiles = 1;
    r.s_chunk = 1;
    r.blocks = ((c.batch ? c.S : c.S * c.P) + 255) / 256;
  }
  r.n = c.S;
  out.mode = r.mode;
  if (!analytical || model.custom) {
    r.solver = analytical ? 0 : static_cast<int32_t>(pmx::solver_row(d.ode_solver) - pmx::kSolvers);
    r.lag = !analytical && !model.user_ode && model.dev.n_lag_slots > 0;
    r.family = !model.custom ? pmx::R_ODE : (analytical ? pmx::R_JIT_ANALYTICAL : (model.user_ode ? pmx::R_JIT_ODE_USER : pmx::R_JIT_ODE));
    if (model.custom && static_launcher() && r.mode == pmx::MODE_GRID && !c.ll) r.family = pmx::R_STATIC_AGRID;
    out.add(r);
    return out;
  }
  r.lag = model.dev.n_lag_slots > 0;
  r.dyn = !r.lag && model.dyn;
  if (r.mode == pmx::MODE_PAIR) {
    r.family = pmx::R_PAIR;
    out.add(r);
    return out;
  }
  int64_t n_walk = c.S;
  if (f.n_chunks > 0) {
    const int64_t n_exact = f.n_chunks_exact, n_loose = f.n_chunks - f.n_chunks_exact;
    Route k = r;
    k.family = pmx::R_CLASSED;
    if (n_exact > 0) {
      // exact classes of a plain model: the pipelined log-likelihood kernel (PMX_TUNE_LL_OLD: the round-2 one, A/B)
      if (!r.lag && !r.dyn && c.ll && f.has_chunk_hdr && !tun.ll_old && c.ll_ld < (int64_t{1} << 28)) k.family = pmx::R_CLASSED_LL;
      out.add(classed_route(k, n_exact, tun));
      k.family = pmx::R_CLASSED;
    }
    if (!r.lag && n_loose > 0) {  // subjects that share a program shape but not its step lengths
      k.loose = true;
      out.add(classed_route(k, n_loose, tun));
    }
    n_walk = f.n_generic;
    r.leftover = true;
    if (n_walk == 0) return out;
  }
  out.add(walker_route(r, model, f, c, n_walk, tun));
  return out;
}

// closure walkers keep 64 landing times per lane; an occasion with more takes the build with the scan path in
// (model->jit_mu held)
int32_t big_lists_code(const pmx_model* model) {
  if (!model->jit_code_big.empty()) return PMX_OK;
  pmx::JitSpec sp = model->jit_spec;
  sp.big_lists = true;
  std::string log;
  if (!pmx::jit_compile(sp, &model->jit_code_big, &log))
    return fail(PMX_ERR_HIP, "hiprtc could not compile the big-lists build of the model:\n" + log);
  return PMX_OK;
}

// hiprtc-compiled model: its module on the population's device, loaded at first use
int32_t jit_module(const pmx_model* model, const pmx_population* pop, const DeviceStream* ds, const pmx::JitModule** out) {
  const pmx_model_desc& d = model->d;
  std::lock_guard<std::mutex> lock(model->jit_mu);
  const bool big = (d.eq_kind == PMX_EQ_ANALYTICAL || model->user_ode) && ds->f.max_lagb_per_list > pmx::kUserLagKept;
  if (big) {
    const int32_t rc = big_lists_code(model);
    if (rc != PMX_OK) return rc;
  }
  auto& modules = big ? model->jit_modules_big : model->jit_modules;
  auto it = modules.find(pop->device);
  if (it == modules.end()) {
    pmx::JitModule mod;
    const hipError_t le = pmx::jit_load(big ? model->jit_code_big : model->jit_code, &mod, model->jit_spec);
    if (le != hipSuccess) return fail(PMX_ERR_HIP, std::string("loading the compiled model: ") + hipGetErrorString(le));
    it = modules.emplace(pop->device, mod).first;
  }
  *out = &it->second;
  return PMX_OK;
}

// ... and the launch of the module's entry point the route names
int32_t launch_jit(const pmx_model* model, const pmx_population* pop, const DeviceStream* ds, pmx::LaunchArgs& a, const Route& r,
                   hipError_t* e) {
  const pmx::JitModule* jm = nullptr;
  const int32_t rc = jit_module(model, pop, ds, &jm);
  if (rc != PMX_OK) return rc;
  // (a dimension the model's kind does not have is index 0: kJitEntries, pmx_jit_source.hpp)
  const int lag = r.lag ? 1 : 0, ll = r.ll ? 1 : 0, ad = pmx::kSolvers[r.solver].solv;
  int32_t s_chunk = r.s_chunk, n_ptiles = r.n_ptiles;
  if (r.family == pmx::R_STATIC_AGRID) {
    const int rc_s = static_launcher()(&a.m, &a.ops, a.theta, a.P, a.S, s_chunk, n_ptiles, a.pred, a.ld, a.status,
                                       static_cast<uint32_t>(r.blocks), r.threads, a.stream);
    *e = rc_s == 0 ? hipSuccess : hipErrorUnknown;
  } else if (r.mode == pmx::MODE_GRID) {
    void* args[] = {&a.m, &a.ops, &a.theta, &a.P, &a.S, &s_chunk, &n_ptiles, &a.pred, &a.ld, &a.status};
    *e = hipModuleLaunchKernel(jm->fn[0][lag][ll][ad], static_cast<uint32_t>(r.blocks), 1, 1, r.threads, 1, 1, 0,
                               static_cast<hipStream_t>(a.stream), args, nullptr);
  } else {
    void* args[] = {&a.m, &a.ops, &a.theta, &a.P, &a.S, &a.batch, &a.pred, &a.ld, &a.status};
    *e = hipModuleLaunchKernel(jm->fn[1][lag][ll][ad], static_cast<uint32_t>(r.blocks), 1, 1, r.threads, 1, 1, 0,
                               static_cast<hipStream_t>(a.stream), args, nullptr);
  }
  return PMX_OK;
}

// the kernel arguments that do not depend on the route: the model (patched for pmx_predict_state_device), the stream's
// device arrays, the caller's buffers
pmx::LaunchArgs launch_args(const pmx_model* model, const pmx_population* pop, const DeviceStream* ds, const Tunables& tun,
                            const double* d_theta, int64_t P, int batch, double* d_pred, int64_t ld, uint8_t* d_status,
                            void* stream, int state_override, uint32_t* d_stats) {
  pmx::LaunchArgs a{};
  a.m = model->dev;
  a.m.solver_stats = d_stats;  // (pmx_predict_stats_device; null otherwise)
  if (state_override >= 0) {  // Prediction::state: every output equation reads the raw amount of one state
    a.m.state_override = state_override;  // (the run-time-compiled walkers read it)
    for (int o = 0; o < PMX_MAX_OUT; ++o) {
      a.m.out[o] = pmx_out{state_override, PMX_SRC_NONE, 0};
      a.m.out_vol_theta[o] = -1;
    }
  }
  a.ops = ds->dev;
  {
    // ODE PAIR kernel, steps per trip of the lane state machine (pmx_ode.hpp ode_pair_body): tools/experiments/steps_per_trip_sweep.sh
    const int64_t n_pairs = batch ? pop->hp.n_subjects : pop->hp.n_subjects * P;
    a.ops.steps_per_trip = tun.steps_per_trip > 0 ? tun.steps_per_trip : (n_pairs <= 131072 ? 48 : 32);
  }
  a.theta = d_theta;
  a.P = batch ? 1 : P;
  a.S = pop->hp.n_subjects;
  a.pred = d_pred;
  a.ld = batch ? 1 : ld;
  a.status = d_status;
  a.batch = batch;
  a.stream = stream;
  a.cls = ds->cls;
  a.steps = ds->steps;
  a.prop_slots = ds->f.prop_slots;
  return a;
}

}  // namespace

extern "C" int32_t pmx_debug_jit_compile_big_lists(const pmx_model* model) {
  if (!model) return fail(PMX_ERR_INVALID_ARGUMENT, "model is null");
  if (!model->custom || !(model->d.eq_kind == PMX_EQ_ANALYTICAL || model->user_ode)) return PMX_OK;
  std::lock_guard<std::mutex> lock(model->jit_mu);
  return big_lists_code(model);
}

// a library kernel's route -> the entry of its family's translation unit
hipError_t pmx::launch_route(const pmx::LaunchArgs& a, const pmx::Route& r) {
  if (a.S <= 0 || (a.P <= 0 && !a.batch)) return hipSuccess;
  switch (r.family) {
    case pmx::R_CLASSED: return pmx::launch_classed(a, r);
    case pmx::R_CLASSED_LL: return pmx::launch_classed_ll(a, r);
    case pmx::R_STEPS: return pmx::launch_steps(a, r);
    case pmx::R_DYN3: return pmx::launch_dyn3(a, r);
    case pmx::R_GRID: return pmx::launch_grid(a, r);
    case pmx::R_PAIR: return pmx::launch_pair(a, r);
    case pmx::R_ODE: return pmx::launch_ode(a, r);  // (r.mode: grid / pair)
    default: return hipErrorInvalidValue;
  }
}

int32_t enqueue(const pmx_model* model, pmx_population* pop, const double* d_theta, int64_t P, int batch, double* d_pred,
                int64_t ld, uint8_t* d_status, void* stream, const LLRequest* llreq, int state_override, uint32_t* d_stats) {
  const pmx_model_desc& d = model->d;
  if (d.n_covariates != pop->hp.n_cov)
    return fail(PMX_ERR_INVALID_ARGUMENT, "model declares " + std::to_string(d.n_covariates) +
                                              " covariates, population carries " + std::to_string(pop->hp.n_cov));
  const Tunables tun = pmx::tunables();  // the one snapshot of this call
  DeviceStream* ds = nullptr;
  int32_t rc = get_stream(pop, key_for(model, tun, pop->hp.has_infusions), tun.cls, &ds);
  if (rc != PMX_OK) return rc;
  // range checks the reference performs inside the event loop
  if (ds->f.max_input_used >= d.ndrugs)
    return fail(PMX_ERR_INPUT_OUT_OF_RANGE, "input " + std::to_string(ds->f.max_input_used) + " >= ndrugs " +
                                                std::to_string(d.ndrugs));  // equation/mod.rs:322-327
  if (pop->hp.max_outeq >= d.nout)
    return fail(PMX_ERR_OUTEQ_OUT_OF_RANGE,
                "outeq " + std::to_string(pop->hp.max_outeq) + " >= nout " + std::to_string(d.nout));
  if (pop->hp.n_subjects == 0) return PMX_OK;

  pmx::LaunchArgs a = launch_args(model, pop, ds, tun, d_theta, P, batch, d_pred, ld, d_status, stream, state_override, d_stats);
  Call call{a.S, P, batch != 0, llreq != nullptr, false, llreq ? llreq->ld : 0, state_override >= 0};
  DeviceStream::LLCache* slot = nullptr;
  struct SlotGuard {  // the slot is released (event recorded on the stream) however this function leaves
    pmx_population* pop;
    DeviceStream::LLCache** slot;
    void* stream;
    ~SlotGuard() {
      if (*slot) release_ll_slot(pop, *slot, stream);
    }
  } slot_guard{pop, &slot, stream};
  if (llreq != nullptr) {
    rc = acquire_ll_slot(model, pop, ds, llreq->em, stream, &slot, batch != 0);
    if (rc != PMX_OK) return rc;
    a.ops.ll_obs = slot->d_obs;
    a.ops.ll_out = llreq->d_ll;
    a.ops.ll_ld = llreq->ld;
    a.cls.cobs = slot->d_cobs;
    a.cls.chunk_obs_off = ds->d_chunk_obs_off;
    if (llreq->d_sigma_err) *llreq->d_sigma_err = slot->d_err;
    call.cens = pop->any_censored;  // (known once the population's observation arrays are on the device)
    for (int q = 0; q < d.nout && q < PMX_MAX_OUT; ++q)
      if (llreq->em[q].kind >= PMX_EM_RES_CONSTANT) call.cens = true;  // residual models fold from the full records too
  }
  const Routes routes = plan_routes(*model, ds->f, call, tun);
  for (int i = 0; i < routes.n; ++i)
    if (routes.r[i].blocks > 0x7fffffffLL) return fail(PMX_ERR_INVALID_ARGUMENT, "grid too large for one launch");
  // Status bytes need no memset before the launch (it cost ~70 us of serialisation per pass): the PAIR and ODE kernels
  // write every pair's byte; the analytical GRID kernels clear a subject's bytes with 8-byte stores when the row
  // length allows (mode 1) and otherwise write every byte too (mode 2).  Every subject is visited: the generic walker
  // owns the subjects no class holds, empty ones included.
  a.cls.zero_status = 0;
  if (d_status != nullptr && routes.mode == pmx::MODE_GRID && d.eq_kind == PMX_EQ_ANALYTICAL)
    a.cls.zero_status = (P % 8 == 0 && reinterpret_cast<uintptr_t>(d_status) % 8 == 0 && (ds->cls.n_chunks == 0 || ds->cls.G <= 8)) ? 1 : 2;
  hipError_t e = hipSuccess;
  for (int i = 0; i < routes.n && e == hipSuccess; ++i) {
    if (!model->custom) e = pmx::launch_route(a, routes.r[i]);
    else if ((rc = launch_jit(model, pop, ds, a, routes.r[i], &e)) != PMX_OK) return rc;
  }
  pmx::set_kernel_name(routes.name());
  if (e != hipSuccess) return fail(PMX_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return PMX_OK;
}

// pmx_compile.cpp — see pmx_compile.hpp.  Host C++ only (no HIP).
#include "pmx_compile.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

namespace pmx {

namespace {

// f64::total_cmp as an integer key (event.rs:301, covariate.rs:191).
inline int64_t total_key(double v) {
  int64_t b;
  std::memcpy(&b, &v, 8);
  b ^= static_cast<int64_t>(static_cast<uint64_t>(b >> 63) >> 1);
  return b;
}

struct ActiveInfusion {
  double time, amount, duration;
  int32_t input;
};

}  // namespace

bool HostPopulation::interpolate(int64_t occ, int32_t cov, double t, double* out) const {
  const int64_t idx = occ * n_cov + cov;
  const int64_t s0 = cov_seg_off[idx], s1 = cov_seg_off[idx + 1];
  if (s0 == s1) return false;
  // linear scan: first segment with from <= t < to (covariate.rs:221-227, :60-64)
  for (int64_t s = s0; s < s1; ++s) {
    if (seg_from[s] <= t && t < seg_to[s]) {
      *out = std::isnan(seg_slope[s]) ? seg_icpt[s] : (seg_slope[s] * t + seg_icpt[s]);
      return true;
    }
  }
  if (t < cov_first_t[idx]) {
    *out = cov_first_v[idx];
    return true;
  }
  if (t >= cov_last_t[idx]) {
    *out = cov_last_v[idx];
    return true;
  }
  return false;
}

int32_t build_host_population(const pmx_population_desc* d, HostPopulation* hp, std::string* err) {
  auto fail = [&](int32_t code, const std::string& m) {
    *err = m;
    return code;
  };
  if (!d) return fail(PMX_ERR_INVALID_ARGUMENT, "null population descriptor");
  if (d->n_subjects < 0 || d->n_occasions < 0 || d->n_events < 0)
    return fail(PMX_ERR_INVALID_ARGUMENT, "negative sizes");
  if (!d->subj_occ_off || !d->occ_ev_off) return fail(PMX_ERR_INVALID_ARGUMENT, "null offset arrays");
  if (d->n_events > 0 && (!d->ev_time || !d->ev_value || !d->ev_duration || !d->ev_kind || !d->ev_io))
    return fail(PMX_ERR_INVALID_ARGUMENT, "null event arrays");
  if (d->n_covariates < 0 || d->n_covariates > PMX_MAX_COVARIATES)
    return fail(PMX_ERR_INVALID_ARGUMENT, "n_covariates out of range");
  const int64_t S = d->n_subjects, NO = d->n_occasions, NE = d->n_events;
  if (d->subj_occ_off[0] != 0 || d->subj_occ_off[S] != NO)
    return fail(PMX_ERR_INVALID_ARGUMENT, "subj_occ_off must span [0, n_occasions]");
  if (d->occ_ev_off[0] != 0 || d->occ_ev_off[NO] != NE)
    return fail(PMX_ERR_INVALID_ARGUMENT, "occ_ev_off must span [0, n_events]");
  for (int64_t s = 0; s < S; ++s)
    if (d->subj_occ_off[s + 1] < d->subj_occ_off[s]) return fail(PMX_ERR_INVALID_ARGUMENT, "subj_occ_off not monotone");
  for (int64_t o = 0; o < NO; ++o)
    if (d->occ_ev_off[o + 1] < d->occ_ev_off[o]) return fail(PMX_ERR_INVALID_ARGUMENT, "occ_ev_off not monotone");

  hp->n_subjects = S;
  hp->n_occasions = NO;
  hp->n_events = NE;
  hp->n_cov = d->n_covariates;
  hp->subj_occ_off.assign(d->subj_occ_off, d->subj_occ_off + S + 1);
  hp->occ_ev_off.assign(d->occ_ev_off, d->occ_ev_off + NO + 1);
  hp->occ_index.resize(NO);
  for (int64_t s = 0; s < S; ++s)
    for (int64_t o = hp->subj_occ_off[s]; o < hp->subj_occ_off[s + 1]; ++o)
      hp->occ_index[o] = d->occ_index ? d->occ_index[o] : static_cast<int32_t>(o - hp->subj_occ_off[s]);

  hp->ev_time.resize(NE);
  hp->ev_value.resize(NE);
  hp->ev_dur.resize(NE);
  hp->ev_kind.resize(NE);
  hp->ev_io.resize(NE);
  std::vector<int64_t> ev_src(static_cast<size_t>(NE), 0);  // sorted position -> caller's event index
  std::vector<int64_t> order;
  for (int64_t o = 0; o < NO; ++o) {
    const int64_t e0 = hp->occ_ev_off[o], e1 = hp->occ_ev_off[o + 1];
    order.resize(e1 - e0);
    std::iota(order.begin(), order.end(), e0);
    if (!d->presorted) {
      // Occasion::sort: stable, time.total_cmp then Observation < Bolus < Infusion (event.rs:292-304)
      std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        const int64_t ka = total_key(d->ev_time[a]), kb = total_key(d->ev_time[b]);
        if (ka != kb) return ka < kb;
        return d->ev_kind[a] < d->ev_kind[b];
      });
    }
    for (int64_t i = 0; i < e1 - e0; ++i) {
      const int64_t src = order[i], dst = e0 + i;
      const uint8_t k = d->ev_kind[src];
      if (k > PMX_EV_INFUSION) return fail(PMX_ERR_INVALID_ARGUMENT, "unknown event kind");
      hp->ev_time[dst] = d->ev_time[src];
      hp->ev_value[dst] = d->ev_value[src];
      hp->ev_dur[dst] = d->ev_duration[src];
      hp->ev_kind[dst] = k;
      hp->ev_io[dst] = d->ev_io[src];
      ev_src[dst] = src;
      if (k == PMX_EV_OBSERVATION)
        hp->max_outeq = std::max<int32_t>(hp->max_outeq, d->ev_io[src]);
      hp->has_infusions |= (k == PMX_EV_INFUSION);
    }
  }
  // prediction rows (event order == flat_predictions order, subject.rs:145-148)
  hp->subj_obs_off.assign(S + 1, 0);
  for (int64_t s = 0; s < S; ++s) {
    const int64_t e0 = hp->occ_ev_off[hp->subj_occ_off[s]], e1 = hp->occ_ev_off[hp->subj_occ_off[s + 1]];
    for (int64_t e = e0; e < e1; ++e)
      if (hp->ev_kind[e] == PMX_EV_OBSERVATION) {
        hp->obs_time.push_back(hp->ev_time[e]);
        hp->obs_value.push_back(hp->ev_value[e]);
        hp->obs_outeq.push_back(hp->ev_io[e]);
        hp->obs_subject.push_back(s);
        if (d->ev_errorpoly)
          for (int c = 0; c < 4; ++c) hp->obs_errorpoly.push_back(d->ev_errorpoly[ev_src[e] * 4 + c]);
        if (d->ev_censor) {
          const int8_t cz = d->ev_censor[ev_src[e]];
          if (cz != PMX_CENSOR_NONE && cz != PMX_CENSOR_BLOQ && cz != PMX_CENSOR_ALOQ)
            return fail(PMX_ERR_INVALID_ARGUMENT, "unknown censoring code");
          hp->obs_censor.push_back(cz);
        }
      }
    hp->subj_obs_off[s + 1] = static_cast<int64_t>(hp->obs_time.size());
  }
  hp->n_obs = static_cast<int64_t>(hp->obs_time.size());

  // covariate segments (Covariate::build_segments, covariate.rs:189-214)
  const int32_t nc = hp->n_cov;
  if (nc > 0) {
    if (!d->cov_knot_off || !d->cov_knot_time || !d->cov_knot_value)
      return fail(PMX_ERR_INVALID_ARGUMENT, "covariate arrays missing");
    const int64_t ncell = NO * nc;
    hp->cov_seg_off.assign(ncell + 1, 0);
    hp->cov_first_t.resize(ncell);
    hp->cov_first_v.resize(ncell);
    hp->cov_last_t.resize(ncell);
    hp->cov_last_v.resize(ncell);
    std::vector<std::pair<double, double>> obs;
    for (int64_t c = 0; c < ncell; ++c) {
      const int64_t k0 = d->cov_knot_off[c], k1 = d->cov_knot_off[c + 1];
      if (k1 <= k0) return fail(PMX_ERR_INVALID_ARGUMENT, "a covariate has no observations in some occasion");
      obs.clear();
      for (int64_t k = k0; k < k1; ++k) obs.emplace_back(d->cov_knot_time[k], d->cov_knot_value[k]);
      std::stable_sort(obs.begin(), obs.end(),
                       [](const auto& a, const auto& b) { return total_key(a.first) < total_key(b.first); });
      const bool fixed = d->cov_fixed && d->cov_fixed[c];
      const size_t n = obs.size();
      for (size_t i = 0; i < n; ++i) {
        const bool has_next = i + 1 < n;
        hp->seg_from.push_back(obs[i].first);
        hp->seg_to.push_back(has_next ? obs[i + 1].first : std::numeric_limits<double>::infinity());
        if (fixed || !has_next) {
          hp->seg_slope.push_back(std::numeric_limits<double>::quiet_NaN());  // CarryForward
          hp->seg_icpt.push_back(obs[i].second);
        } else {
          const double slope = (obs[i + 1].second - obs[i].second) / (obs[i + 1].first - obs[i].first);
          hp->seg_slope.push_back(slope);
          hp->seg_icpt.push_back(obs[i].second - slope * obs[i].first);
        }
      }
      hp->cov_seg_off[c + 1] = static_cast<int64_t>(hp->seg_from.size());
      hp->cov_first_t[c] = obs.front().first;
      hp->cov_first_v[c] = obs.front().second;
      hp->cov_last_t[c] = obs.back().first;
      hp->cov_last_v[c] = obs.back().second;
    }
  }
  return PMX_OK;
}

// ------------------------------------------------------------------------------------
// op stream
// ------------------------------------------------------------------------------------
namespace {

// Lagged boluses leave the event list (the device merges them at t + lag(theta)); what remains is walked exactly like
// before.  Slot k = the k-th lagged input, or the one list all inputs of a lag_merge key share.
struct LagLists {
  int32_t slot_of_input[PMX_MAX_INPUTS];
  int32_t n_slots = 0;

  explicit LagLists(const CompileKey& key) {
    for (int i = 0; i < PMX_MAX_INPUTS; ++i)
      slot_of_input[i] = ((key.lag_mask >> i) & 1u) ? (key.lag_merge ? 0 : n_slots++) : -1;
    if (key.lag_merge && key.lag_mask != 0) n_slots = 1;
  }
  bool is_lagged(const HostPopulation& hp, int64_t e) const {
    return n_slots > 0 && hp.ev_kind[e] == PMX_EV_BOLUS && hp.ev_io[e] < PMX_MAX_INPUTS && slot_of_input[hp.ev_io[e]] >= 0;
  }
  int64_t next_kept(const HostPopulation& hp, int64_t e, int64_t e1) const {  // first event of [e, e1) that stays in the list
    while (e < e1 && is_lagged(hp, e)) ++e;
    return e;
  }
  // Lists the lagged boluses of occasion [e0, e1) per slot, in event order, and notes on the occasion's RESET op what a
  // lane needs to know of the remaining list: op_t0 = the time of its first event (+inf: none) and, in First, its kind.
  // ODE: which event is FIRST in the re-sorted list decides what is applied at the solver clock without integration
  // (pmx_ode.hpp "the solver clock"); at equal times a bolus sorts behind an observation and in front of an infusion
  // (event.rs:292-304).
  void extract(const HostPopulation& hp, int64_t e0, int64_t e1, size_t reset_op, OpStream* os) const {
    const int64_t first = next_kept(hp, e0, e1);
    os->op_t0[reset_op] = first < e1 ? hp.ev_time[first] : std::numeric_limits<double>::infinity();
    os->op_meta[reset_op] |= (first < e1 ? static_cast<uint32_t>(hp.ev_kind[first]) : 3u) << kOpFirstShift;
    for (int32_t k = 0; k < n_slots; ++k) {
      const int64_t before = static_cast<int64_t>(os->lagb_time.size());
      for (int64_t e = e0; e < e1; ++e) {
        if (!is_lagged(hp, e) || slot_of_input[hp.ev_io[e]] != k) continue;
        os->max_input_used = std::max<int32_t>(os->max_input_used, hp.ev_io[e]);
        os->lagb_time.push_back(hp.ev_time[e]);
        os->lagb_amount.push_back(hp.ev_value[e]);
        os->lagb_input.push_back(hp.ev_io[e]);
      }
      os->lagb_off.push_back(static_cast<int64_t>(os->lagb_time.size()));
      os->max_lagb_per_list = std::max(os->max_lagb_per_list, os->lagb_off.back() - before);
    }
  }
};

// Appends ops: one method per kind, each filling every column the stream carries for this key.
struct OpWriter {
  const HostPopulation& hp;
  const CompileKey& key;
  OpStream* os;
  const bool ode, times;  // times: ops carry absolute [t0, t1) (PROP) / the first event's time (RESET)
  std::vector<double> covv;
  bool cov_missing = false;

  OpWriter(const HostPopulation& hp_, const CompileKey& key_, OpStream* os_, bool times_)
      : hp(hp_), key(key_), os(os_), ode(key_.eq_kind == PMX_EQ_ODE), times(times_), covv(hp_.n_cov > 0 ? hp_.n_cov : 1, 0.0) {}

  // initial_state: zeros, init only for occasion index 0 (analytical/mod.rs:409-426); op_a = the global occasion index
  size_t reset(int64_t occ) {
    put(OP_RESET, hp.occ_index[occ] == 0 ? 1u : 0u, static_cast<double>(occ), 0.0, 0, nullptr);
    no_covariates();
    return os->op_meta.size() - 1;
  }
  void bolus(int64_t e) {  // (op_b: its time, for a user fa / bolus jump)
    os->max_input_used = std::max<int32_t>(os->max_input_used, hp.ev_io[e]);
    put(OP_BOLUS, hp.ev_io[e], hp.ev_value[e], hp.ev_time[e], 0, nullptr);
    no_covariates();
  }
  void obs(int64_t occ, int64_t e) {
    put(OP_OBS, hp.ev_io[e], hp.ev_time[e], 0.0, 0, nullptr);
    covariates_at(occ, hp.ev_time[e]);
  }
  // one constant-rate piece [t0, t1): b = rateiv[0] (analytical) / the RK4 step (ODE, n of them); `rates`: every input's
  // rate (ODE and full_rates streams); covariates are evaluated at t_cov
  void prop(int64_t occ, double t0, double t1, double b, int32_t n, const double* rates, double t_cov) {
    put(OP_PROP, 0, t1 - t0, b, n, rates);
    covariates_at(occ, t_cov);
    if (times) {
      os->op_t0.back() = t0;
      os->op_t1.back() = t1;
    }
    os->n_prop++;
  }

 private:
  void put(uint32_t kind, uint32_t io, double a, double b, int32_t n, const double* rates) {
    os->op_meta.push_back(make_meta(kind, io));
    os->op_a.push_back(a);
    os->op_b.push_back(b);
    if (times) {
      os->op_t0.push_back(0.0);
      os->op_t1.push_back(0.0);
    }
    if (ode) os->op_n.push_back(n);
    if (ode || key.full_rates)
      for (int32_t r = 0; r < key.n_rate; ++r) os->op_rate.push_back(rates ? rates[r] : 0.0);
  }
  void no_covariates() {  // RESET, BOLUS: zero covariates, unit factors
    if (hp.n_cov == 0 || key.user_cov) return;
    os->op_cov.insert(os->op_cov.end(), static_cast<size_t>(hp.n_cov), 0.0);
    os->op_fac.insert(os->op_fac.end(), static_cast<size_t>(key.n_derived) * PMX_MAX_FACTORS, 1.0);
  }
  // the covariates an OBS / PROP sees and the factors of every derived value at them (expand/analytical.rs:254,286;
  // bindings.rs:98-117), written exactly like the per-lane expression they replace
  void covariates_at(int64_t occ, double t) {
    if (hp.n_cov == 0 || key.user_cov) return;
    for (int32_t c = 0; c < hp.n_cov; ++c) {
      double v = 0.0;
      if (!hp.interpolate(occ, c, t, &v)) cov_missing = true;
      os->op_cov.push_back(v);
      covv[c] = v;
    }
    for (int32_t d = 0; d < key.n_derived; ++d)
      for (int32_t k = 0; k < PMX_MAX_FACTORS; ++k) {
        double fac = 1.0;
        if (k < key.derived[d].n_factors) {
          const pmx_factor& f = key.derived[d].f[k];
          const double cv = covv[f.cov];
          fac = (f.op == PMX_F_POW) ? std::pow(cv / f.ref, f.coef) : (1.0 + f.coef * (cv - f.ref));
        }
        os->op_fac.push_back(fac);
      }
  }
};

// The occasion walks: the events of one occasion -> ops.
struct OccasionWalker {
  const HostPopulation& hp;
  const CompileKey& key;
  OpStream* os;
  LagLists lag;
  OpWriter w;
  std::vector<ActiveInfusion> inf;
  std::vector<double> ts, bounds, rate;

  OccasionWalker(const HostPopulation& hp_, const CompileKey& key_, OpStream* os_)
      : hp(hp_), key(key_), os(os_), lag(key_), w(hp_, key_, os_, lag.n_slots > 0 || key_.want_times),
        rate(key_.n_rate > 0 ? key_.n_rate : 1, 0.0) {}

  int32_t walk(int64_t occ, std::string* err) {
    const int64_t e0 = hp.occ_ev_off[occ], e1 = hp.occ_ev_off[occ + 1];
    const size_t reset_op = w.reset(occ);
    inf.clear();
    if (lag.n_slots > 0) lag.extract(hp, e0, e1, reset_op, os);
    if (w.ode) return walk_ode(occ, e0, e1, reset_op, err);
    walk_analytical(occ, e0, e1);
    return PMX_OK;
  }

 private:
  void push_infusion(int64_t e) { inf.push_back({hp.ev_time[e], hp.ev_value[e], hp.ev_dur[e], static_cast<int32_t>(hp.ev_io[e])}); }

  void walk_analytical(int64_t occ, int64_t e0, int64_t e1) {  // simulate_event, equation/mod.rs:300-358
    for (int64_t e = lag.next_kept(hp, e0, e1); e < e1;) {
      const uint8_t k = hp.ev_kind[e];
      if (k == PMX_EV_BOLUS) {
        w.bolus(e);
      } else if (k == PMX_EV_INFUSION) {
        push_infusion(e);
      } else {
        // Lag models: the lagged boluses are not in this list; the device merges them into the PROP steps at their
        // landing times.  An observation that no PROP step precedes (events closer than the solve's 1e-12 dedup, or
        // at the same instant) can still have a lagged bolus landing in front of it - a zero lag leaves the bolus
        // where it was recorded, between two observations one ulp apart (found by the fuzz suite: seed 2235).  Flush
        // tells the device to take the boluses landing before this observation's time first.
        const bool flush = lag.n_slots > 0 && op_kind(os->op_meta.back()) != OP_PROP;
        w.obs(occ, e);
        if (flush) os->op_meta.back() |= 1u << kOpFlushShift;
      }
      const int64_t en = lag.next_kept(hp, e + 1, e1);
      if (en < e1) solve_analytical(occ, hp.ev_time[e], hp.ev_time[en]);
      e = en;
    }
  }

  // Analytical::solve over [ti, tf] (analytical/mod.rs:299-370): one PROP per constant-rate sub-segment
  void solve_analytical(int64_t occ, double ti, double tf) {
    if (ti == tf) return;  // :308-310
    ts.clear();
    ts.push_back(ti);
    ts.push_back(tf);
    for (const auto& f : inf) {  // :316-325 strictly-inside breakpoints
      const double t0 = f.time, t1 = t0 + f.duration;
      if (t0 > ti && t0 < tf) ts.push_back(t0);
      if (t1 > ti && t1 < tf) ts.push_back(t1);
    }
    std::sort(ts.begin(), ts.end());  // :326
    size_t n = 1;                     // dedup_by |a-b| < 1e-12 against the last retained, :327
    for (size_t r = 1; r < ts.size(); ++r)
      if (!(std::fabs(ts[r] - ts[n - 1]) < 1e-12)) ts[n++] = ts[r];
    for (size_t i = 1; i < n; ++i) {  // :334-367
      const double cur = ts[i - 1], nxt = ts[i];
      double r0 = 0.0;  // rateiv[0]: the only slot the closed forms read
      if (key.full_rates) std::fill(rate.begin(), rate.end(), 0.0);
      for (const auto& f : inf) {
        const double st = f.time, en = st + f.duration;
        if (cur >= st && nxt <= en) {
          os->max_input_used = std::max(os->max_input_used, f.input);
          if (f.input == key.rate_input) r0 += f.amount / f.duration;  // :355
          if (key.full_rates && f.input < key.n_rate) rate[f.input] += f.amount / f.duration;
        }
      }
      const double t_cov = key.cov_time_mode == PMX_COV_TIME_SEGMENT_END_ABS ? nxt : nxt - cur;
      w.prop(occ, cur, nxt, r0, 0, key.full_rates ? rate.data() : nullptr, t_cov);
      if (key.solve_marks && i > 1) os->op_meta.back() |= 1u << kOpContinuesShift;
    }
  }

  // ODE::run_events (ode/mod.rs:609-823) with InfusionSchedule over ALL infusions of the occasion (closure.rs:109-180)
  int32_t walk_ode(int64_t occ, int64_t e0, int64_t e1, size_t reset_op, std::string* err) {
    bounds.clear();
    for (int64_t e = e0; e < e1; ++e) {
      if (hp.ev_kind[e] != PMX_EV_INFUSION) continue;
      if (hp.ev_dur[e] <= 0.0) continue;  // closure.rs:127-129
      os->max_input_used = std::max<int32_t>(os->max_input_used, hp.ev_io[e]);
      push_infusion(e);
      bounds.push_back(hp.ev_time[e]);
      bounds.push_back(hp.ev_time[e] + hp.ev_dur[e]);
    }
    std::sort(bounds.begin(), bounds.end());
    bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());  // exact dedup, closure.rs:143-148
    // The solver clock starts at Occasion::initial_time() of the occasion AS RECORDED - lagged boluses at their
    // recorded times included (ode/mod.rs:348 takes it from the occasion, not from the lag-rewritten event list;
    // structs.rs:782-793) - and only moves forward to the time of the next event (ode/mod.rs:719-721).  PROP ops
    // therefore start there; a lane whose own clock is ahead (boluses that landed before the first remaining event
    // took it there) starts its piece at its clock (pmx_ode.hpp / pmx_ode_user.hpp).  RESET: op_b = that time.
    double t = 0.0;
    for (int64_t e = e0; e < e1; ++e) t = (e == e0) ? hp.ev_time[e] : std::min(t, hp.ev_time[e]);
    os->op_b[reset_op] = t;
    size_t bcur = 0;
    for (int64_t e = lag.next_kept(hp, e0, e1); e < e1;) {
      if (hp.ev_kind[e] == PMX_EV_BOLUS) w.bolus(e);
      if (hp.ev_kind[e] == PMX_EV_OBSERVATION) w.obs(occ, e);
      const int64_t en = lag.next_kept(hp, e + 1, e1);
      const double next_t = en < e1 ? hp.ev_time[en] : t;
      while (next_t > t) {  // ode/mod.rs:721-739
        while (bcur < bounds.size() && bounds[bcur] <= t) ++bcur;
        double stop = next_t;
        if (bcur < bounds.size() && bounds[bcur] <= next_t) stop = bounds[bcur++];
        std::fill(rate.begin(), rate.end(), 0.0);
        for (const auto& f : inf)  // right-continuous rate at t (closure.rs:80-99)
          if (f.time <= t && t < f.time + f.duration && f.input < key.n_rate) rate[f.input] += f.amount / f.duration;
        const double dt = stop - t;
        if (dt > 0.0) {
          double nf = std::ceil(dt / key.rk4_h_max);
          if (nf < 1.0) nf = 1.0;
          if (nf > 2.0e9) {
            *err = "RK4 step count overflow (dt / rk4_h_max too large)";
            return PMX_ERR_INVALID_ARGUMENT;
          }
          const int32_t n = static_cast<int32_t>(nf);
          w.prop(occ, t, stop, dt / static_cast<double>(n), n, rate.data(), t);
        }
        t = stop;
      }
      e = en;
    }
    return PMX_OK;
  }
};

// Propagator reuse for covariate-derived rate constants, one occasion's PROP ops `props` at a time (a RESET re-derives
// the lane's failure state).  The macro lowering evaluates `derive` at the segment LENGTH (expand/analytical.rs:254,286),
// so two PROPs of equal length see equal covariates, hence equal rate constants and the same transition matrix (a
// subject-constant covariate gives the same under either rule).  Key = (dt, factor row) bitwise; a key with a later
// use gets a slot (furthest-next-use eviction).  Cache code: 1 + k = build and keep in slot k, 1 + S + k = take slot k
// (S = prop_cache_slots), 0 = build.
void code_prop_cache(const std::vector<int64_t>& props, int32_t n_slots, size_t nfac, OpStream* os) {
  auto same_row = [&](int64_t a, int64_t b) {
    return std::memcmp(&os->op_fac[static_cast<size_t>(a) * nfac], &os->op_fac[static_cast<size_t>(b) * nfac], nfac * 8) == 0;
  };
  auto same = [&](int64_t a, int64_t b) {  // (rate-free segments keep the transition part only: they share among
    // themselves, segments under an infusion likewise)
    return std::memcmp(&os->op_a[a], &os->op_a[b], 8) == 0 && (os->op_b[a] != 0.0) == (os->op_b[b] != 0.0) && same_row(a, b);
  };
  const size_t n = props.size();
  std::vector<int64_t> next(n, -1);  // index (into props) of the next PROP with the same key
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j)
      if (same(props[i], props[j])) {
        next[i] = static_cast<int64_t>(j);
        break;
      }
  int64_t last_built = -1;
  std::vector<int64_t> holder(static_cast<size_t>(n_slots), -1);  // slot -> index of the PROP whose propagator it holds
  for (size_t i = 0; i < n; ++i) {
    int32_t from = -1;
    for (int32_t k = 0; k < n_slots; ++k)
      if (holder[k] >= 0 && next[static_cast<size_t>(holder[k])] == static_cast<int64_t>(i)) from = k;
    uint32_t code = 0;
    if (from >= 0) {  // take it; the slot now stands for this PROP (same key, next use continues the chain)
      code = static_cast<uint32_t>(1 + n_slots + from);
      holder[from] = next[i] >= 0 ? static_cast<int64_t>(i) : -1;
      os->n_prop_reused++;
      os->prop_cache_used = std::max(os->prop_cache_used, from + 1);
    } else if (next[i] >= 0) {  // first of several: keep it if a slot is free or holds something needed later than this
      int32_t pick = -1;
      int64_t worst = -1;
      for (int32_t k = 0; k < n_slots; ++k) {
        const int64_t h = holder[k];
        if (h < 0) {
          pick = k;
          worst = std::numeric_limits<int64_t>::max();
          break;
        }
        if (next[static_cast<size_t>(h)] > worst) {
          worst = next[static_cast<size_t>(h)];
          pick = k;
        }
      }
      if (pick >= 0 && (holder[pick] < 0 || worst > next[i])) {
        holder[pick] = static_cast<int64_t>(i);
        code = static_cast<uint32_t>(1 + pick);
      }
    }
    os->op_meta[props[i]] |= code << kOpCacheShift;
    // SameFac: this PROP's covariate factor row equals the one of the occasion's previous BUILT PROP (a subject-constant
    // covariate: every segment) - the rate constants, hence the eigenvalues, are the same and only the step length
    // differs (pmx_analytical_dyn3 keeps the last eigenvalues in registers).  "Built" = not taken from a slot.
    if (code <= static_cast<uint32_t>(n_slots)) {
      if (last_built >= 0 && same_row(props[i], last_built)) os->op_meta[props[i]] |= kOpSameFacBit;
      last_built = props[i];
    }
  }
}

// cache codes of the ops [o0, o1) of one subject, occasion by occasion
void code_prop_cache_of_subject(const CompileKey& key, int64_t o0, int64_t o1, OpStream* os) {
  const size_t nfac = static_cast<size_t>(key.n_derived) * PMX_MAX_FACTORS;
  std::vector<int64_t> props;
  for (int64_t o = o0; o <= o1; ++o) {
    if (o == o1 || op_kind(os->op_meta[o]) == OP_RESET) {
      code_prop_cache(props, key.prop_cache_slots, nfac, os);
      props.clear();
    } else if (op_kind(os->op_meta[o]) == OP_PROP) {
      props.push_back(o);
    }
  }
}

// exponential ladder along one subject's PROP ops (the lane's rate constants never change)
void code_ladder(int64_t o0, int64_t o1, OpStream* os) {
  double prev = 0.0, span = 1.0;
  for (int64_t o = o0; o < o1; ++o)
    if (op_kind(os->op_meta[o]) == OP_PROP) os->op_meta[o] |= ladder_code(os->op_a[o], &prev, &span) << kOpRungShift;
}

// lane-per-pair kernels: neighbours in a wavefront should have similar op counts (ODE: RK4 step counts)
void order_subjects(int64_t n_subjects, OpStream* os) {
  std::vector<int64_t> work(n_subjects);
  int64_t longest = 0;
  for (int64_t s = 0; s < n_subjects; ++s) {
    const int64_t o0 = os->subj_op_off[s], o1 = os->subj_op_off[s + 1];
    work[s] = o1 - o0;
    for (int64_t o = o0; o < o1 && !os->op_n.empty(); ++o) work[s] += os->op_n[o];
    longest = std::max(longest, o1 - o0);
  }
  os->subj_order.resize(n_subjects);
  std::iota(os->subj_order.begin(), os->subj_order.end(), 0);
  std::stable_sort(os->subj_order.begin(), os->subj_order.end(), [&](int32_t a, int32_t b) { return work[a] > work[b]; });
  os->max_ops_per_subject = static_cast<int32_t>(longest);
}

}  // namespace

int32_t compile_ops(const HostPopulation& hp, const CompileKey& key, OpStream* os, std::string* err) {
  *os = OpStream{};
  os->key = key;
  os->subj_op_off.assign(hp.n_subjects + 1, 0);
  OccasionWalker walker(hp, key, os);
  os->n_lag_slots = walker.lag.n_slots;
  if (os->n_lag_slots > 0) os->lagb_off.push_back(0);
  const bool analytical = key.eq_kind != PMX_EQ_ODE;
  for (int64_t s = 0; s < hp.n_subjects; ++s) {
    for (int64_t occ = hp.subj_occ_off[s]; occ < hp.subj_occ_off[s + 1]; ++occ) {
      const int32_t rc = walker.walk(occ, err);
      if (rc != PMX_OK) return rc;
    }
    const int64_t o0 = os->subj_op_off[s], o1 = static_cast<int64_t>(os->op_meta.size());
    os->subj_op_off[s + 1] = o1;
    if (analytical && key.prop_cache_slots > 0 && !os->op_fac.empty()) code_prop_cache_of_subject(key, o0, o1, os);
    if (analytical && key.ladder) code_ladder(o0, o1, os);
  }
  if (walker.w.cov_missing) {
    *err = "covariate interpolation failed (MissingSegments)";
    return PMX_ERR_INVALID_ARGUMENT;
  }
  os->n_ops = static_cast<int64_t>(os->op_meta.size());
  order_subjects(hp.n_subjects, os);
  return PMX_OK;
}

}  // namespace pmx

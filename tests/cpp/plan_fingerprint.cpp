// plan_fingerprint — byte-level fingerprint of everything the population compiler produces.
//
// Stand-alone host program: pmx_compile.hpp and the host compiler sources only (no HIP, no libpmx_hip.so, no Python).
// For every case of a fixed corpus of (population, CompileKey) pairs it runs build_host_population + plan_stream and
// prints one line per field of StreamPlan / OpStream / ClassPlan:
//
//   <case> <field> <element count> <64-bit FNV-1a of the raw bytes>
//
// tests/golden/plan_fingerprints.txt holds that output (tests/test_plan_fingerprint.py compares line by line, so a
// mismatch names the array that moved).  The corpus uses its own integer generator and only arithmetic whose result
// is fixed by IEEE-754 (power factors see power-of-two ratios and small integer exponents), so the fixture does not
// depend on the C++ library or libm of the machine that runs it.
//
//   plan_fingerprint            print the fingerprints
//   plan_fingerprint --time N   plan a C3-shaped and a C5-shaped population N times each; best / median milliseconds
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "pmx_compile.hpp"

namespace {

// ---- generator ----------------------------------------------------------------------------------------------------
struct Rng {  // splitmix64
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
  int below(int n) { return static_cast<int>(next() % static_cast<uint64_t>(n)); }
  double unit() { return static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1), exact
  double grid(int n, double step) { return below(n) * step; }                               // k * step, k < n
};

// ---- population builder -------------------------------------------------------------------------------------------
struct Pop {
  std::vector<int64_t> subj_occ_off{0}, occ_ev_off{0}, knot_off{0};
  std::vector<int32_t> occ_index;
  std::vector<double> t, v, dur, kt, kv;
  std::vector<uint8_t> kind, fixed;
  std::vector<uint16_t> io;
  int32_t n_cov = 0;
  bool presorted = false;
  int32_t next_index = 0;

  void ev(uint8_t k, double time, double value, double d, int i) {
    kind.push_back(k);
    t.push_back(time);
    v.push_back(value);
    dur.push_back(d);
    io.push_back(static_cast<uint16_t>(i));
  }
  void obs(double time, int outeq = 0) { ev(PMX_EV_OBSERVATION, time, 0.0, 0.0, outeq); }
  void bolus(double time, double amt, int input = 0) { ev(PMX_EV_BOLUS, time, amt, 0.0, input); }
  void infusion(double time, double amt, double d, int input = 0) { ev(PMX_EV_INFUSION, time, amt, d, input); }
  // one covariate of the occasion being built (call n_cov times per occasion, before end_occasion)
  void cov(std::initializer_list<std::pair<double, double>> knots, bool carry = false) {
    for (const auto& k : knots) {
      kt.push_back(k.first);
      kv.push_back(k.second);
    }
    knot_off.push_back(static_cast<int64_t>(kt.size()));
    fixed.push_back(carry ? 1 : 0);
  }
  void end_occasion() {
    occ_ev_off.push_back(static_cast<int64_t>(t.size()));
    occ_index.push_back(next_index++);
  }
  void end_subject() {
    subj_occ_off.push_back(static_cast<int64_t>(occ_index.size()));
    next_index = 0;
  }
  pmx_population_desc desc() const {
    pmx_population_desc d{};
    d.n_subjects = static_cast<int64_t>(subj_occ_off.size()) - 1;
    d.n_occasions = static_cast<int64_t>(occ_index.size());
    d.n_events = static_cast<int64_t>(t.size());
    d.subj_occ_off = subj_occ_off.data();
    d.occ_ev_off = occ_ev_off.data();
    d.occ_index = occ_index.data();
    d.ev_time = t.data();
    d.ev_value = v.data();
    d.ev_duration = dur.data();
    d.ev_kind = kind.data();
    d.ev_io = io.data();
    d.n_covariates = n_cov;
    d.presorted = presorted ? 1 : 0;
    if (n_cov > 0) {
      d.cov_knot_off = knot_off.data();
      d.cov_knot_time = kt.data();
      d.cov_knot_value = kv.data();
      d.cov_fixed = fixed.data();
    }
    return d;
  }
};

// ---- populations --------------------------------------------------------------------------------------------------
constexpr double kDesignT[7] = {0.5, 1.0, 2.0, 4.0, 8.0, 12.0, 24.0};

// C3-like protocol: infusion(0, amount_s, 0.5) + 7 observations; `jitter`: each subject's own sampling times
void add_design(Pop* p, int n, Rng* rng, bool jitter, int n_obs = 7, double dur = 0.5) {
  for (int s = 0; s < n; ++s) {
    p->infusion(0.0, 500.0 + s, dur);
    for (int i = 0; i < n_obs; ++i) p->obs(kDesignT[i] * (jitter && i > 0 ? 1.0 + (rng->below(201) - 100) / 1024.0 : 1.0));
    p->end_occasion();
    p->end_subject();
  }
}

// 21 subjects on one protocol: exact classes, the last chunk of 8 (or 4) partly full
Pop pop_shared() {
  Pop p;
  Rng rng(1);
  add_design(&p, 21, &rng, false);
  return p;
}

// jittered times (the infusion ends strictly inside the second interval): a loose class of 12 + the three subjects on
// the exact protocol, which are too few for a class of their own (two chunks, the second partly full), and a shape
// with 5 members, below the 3/4-full cut of G = 8: generic
Pop pop_jitter() {
  Pop p;
  Rng rng(2);
  add_design(&p, 12, &rng, true, 7, 0.75);
  add_design(&p, 5, &rng, true, 5, 0.75);
  add_design(&p, 3, &rng, false, 7, 0.75);
  return p;
}

// ragged random subjects: 0..3 occasions of 0..12 events on a coarse time grid (equal times are common), inputs 0..2,
// outputs 0..1, presorted off so the library's own sort runs
Pop pop_ragged(uint64_t seed, int n) {
  Pop p;
  Rng rng(seed);
  for (int s = 0; s < n; ++s) {
    const int n_occ = rng.below(4);
    for (int o = 0; o < n_occ; ++o) {
      const int n_ev = rng.below(13);
      for (int e = 0; e < n_ev; ++e) {
        const int k = rng.below(10);
        const double time = rng.grid(25, 0.5) + (rng.below(4) == 0 ? rng.unit() : 0.0);
        if (k < 5)
          p.obs(time, rng.below(2));
        else if (k < 8)
          p.bolus(time, 10.0 + rng.below(90), rng.below(3));
        else
          p.infusion(time, 100.0 + rng.below(400), 0.25 + rng.grid(12, 0.25), rng.below(3));
      }
      p.end_occasion();
    }
    p.end_subject();
  }
  return p;
}

// hand-made subjects, one branch each
Pop pop_edges() {
  Pop p;
  p.end_subject();  // no occasion at all: an empty subject
  p.end_occasion();  // an occasion without events
  p.end_subject();
  p.bolus(0.0, 100.0);  // doses only
  p.infusion(1.0, 50.0, 2.0, 1);
  p.end_occasion();
  p.end_subject();
  // overlapping infusions; one ends strictly inside (4, 6); a zero-length infusion
  p.infusion(0.0, 100.0, 3.0);
  p.infusion(1.0, 60.0, 4.0);
  p.infusion(2.0, 10.0, 0.0, 1);
  p.infusion(2.5, 30.0, 1.0, 1);
  p.obs(2.0);
  p.obs(4.0);
  p.obs(6.0, 1);
  p.end_occasion();
  p.end_subject();
  // breakpoints closer than 1e-12 to each other and to the interval's end: dropped by the dedup
  p.obs(0.0);
  p.infusion(0.0, 10.0, 1.0);
  p.infusion(0.25, 10.0, 0.75 + 5e-13);
  p.infusion(0.5, 10.0, 1.5 - 3e-13);
  p.obs(2.0);
  p.obs(2.0 + 4e-13);  // no PROP between these two
  p.obs(3.0);
  p.end_occasion();
  p.end_subject();
  // equal times: observation < bolus < infusion; two observations at one instant (an OP_OBS step of its own)
  p.infusion(1.0, 10.0, 1.0);
  p.bolus(1.0, 5.0);
  p.obs(1.0);
  p.obs(1.0, 1);
  p.bolus(0.0, 7.0, 1);
  p.obs(2.0);
  p.obs(2.0);
  p.obs(2.0, 1);
  p.end_occasion();
  // the subject's second and third occasion (init runs for index 0 only); the third starts with observations
  p.bolus(0.0, 1.0);
  p.obs(1.0);
  p.end_occasion();
  p.obs(0.0);
  p.obs(0.0);
  p.bolus(0.5, 2.0, 1);
  p.obs(1.5);
  p.end_occasion();
  p.end_subject();
  return p;
}

// 9 subjects, 70 observations one hour apart + a late infusion: programs past bit 63 of both masks
Pop pop_long() {
  Pop p;
  p.presorted = true;
  for (int s = 0; s < 9; ++s) {
    p.bolus(0.0, 100.0 + s);
    for (int i = 1; i <= 70; ++i) {
      if (i == 66) p.infusion(65.0, 10.0 + s, 2.0);
      p.obs(static_cast<double>(i));
    }
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// step lengths 1, 1, 2, 4, ... 8192: the ladder's span passes 1024 and restarts; then 3x, 4x, 5x rungs
Pop pop_ladder() {
  Pop p;
  for (int s = 0; s < 5; ++s) {
    p.bolus(0.0, 10.0 + s);
    double time = 0.0, dt = 1.0;
    p.obs(time += dt);
    for (int i = 0; i < 14; ++i) {
      p.obs(time += dt);
      dt *= 2.0;
    }
    dt = 3.0;
    p.obs(time += dt);
    p.obs(time += 3.0 * dt);
    p.obs(time += 12.0 * dt);
    p.obs(time += 60.0 * dt);
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// pm_ indexing: infusions into input 1 carry the rate; every third subject doses into input 0 (the pad slot) - four of
// them, enough for a class if the plan did not leave them to the generic walker
Pop pop_pm() {
  Pop p;
  for (int s = 0; s < 12; ++s) {
    p.infusion(0.0, 100.0 + s, 1.0, 1);
    p.bolus(0.0, 20.0, s % 3 == 0 ? 0 : 1);
    p.infusion(2.0, 50.0, 1.0, s % 2);  // input 0: not the closed form's rate
    for (int i = 1; i <= 4; ++i) p.obs(static_cast<double>(i));
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// lag models: boluses on inputs 0 and 1 (which are lagged is the key's business), an unlagged input 2
void lag_occasion(Pop* p, int first) {  // first remaining event: 0 observation, 1 bolus, 2 infusion, 3 none
  p->bolus(0.0, 100.0, 0);
  p->bolus(0.0, 40.0, 1);
  if (first == 0) p->obs(0.0);
  if (first == 1) p->bolus(0.0, 5.0, 2);
  if (first == 2) p->infusion(0.0, 30.0, 1.5, 2);
  if (first != 3) {
    p->obs(1.0);
    p->bolus(1.0, 50.0, 0);  // recorded between two observations with no PROP between them
    p->obs(1.0, 1);
    p->obs(2.0);
    p->bolus(2.0 + 2e-13, 25.0, 1);
    p->obs(2.0 + 4e-13);
    p->obs(4.0);
    p->bolus(5.0, 10.0, 0);  // a lagged bolus behind the last remaining event
  }
  p->end_occasion();
}
Pop pop_lag() {
  Pop p;
  for (int s = 0; s < 9; ++s) {  // a shared design: one exact lag class of 9
    for (int first = 0; first < 4; ++first) lag_occasion(&p, first);
    p.end_subject();
  }
  for (int s = 0; s < 4; ++s) {  // the same ops with their own bolus times: another class
    p.bolus(0.25, 100.0, 0);
    p.obs(1.0);
    p.obs(3.0);
    p.end_occasion();
    p.end_subject();
  }
  for (int s = 0; s < 2; ++s) {  // too few to batch
    p.bolus(0.5, 100.0, 0);
    p.obs(1.0);
    p.obs(3.0);
    p.end_occasion();
    p.end_subject();
  }
  Rng rng(7);
  for (int s = 0; s < 6; ++s) {  // ragged
    const int n_occ = 1 + rng.below(2);
    for (int o = 0; o < n_occ; ++o) {
      const int n_ev = 1 + rng.below(9);
      for (int e = 0; e < n_ev; ++e) {
        const int k = rng.below(8);
        const double time = rng.grid(13, 0.5);
        if (k < 3)
          p.obs(time, rng.below(2));
        else if (k < 7)
          p.bolus(time, 10.0 + rng.below(90), rng.below(3));
        else
          p.infusion(time, 100.0, 0.5 + rng.grid(4, 0.5), 2);
      }
      p.end_occasion();
    }
    p.end_subject();
  }
  return p;
}

// covariates: `wt` (linear in time, or one knot = subject-constant) feeds a LIN factor; `size` is carried forward
// between power-of-two values and feeds the POW factors.  Steps repeat 1, 2, 3 so propagators can be reused and evicted.
Pop pop_cov() {
  Pop p;
  p.n_cov = 2;
  Rng rng(11);
  auto occasion = [&](int s, bool infuse, int n_obs) {
    p.bolus(0.0, 100.0 + s);
    if (infuse) p.infusion(6.0, 60.0, 6.0);
    double time = 0.0;
    for (int i = 0; i < n_obs; ++i) p.obs(time += 1.0 + i % 3);
    if (s % 3 == 0)
      p.cov({{0.0, 60.0 + s}});  // subject-constant
    else
      p.cov({{0.0, 50.0 + rng.below(40)}, {8.0, 60.0 + rng.below(40)}, {20.0, 55.0 + rng.below(40)}});
    if (s % 2 == 0)
      p.cov({{0.0, 140.0}}, true);
    else
      p.cov({{0.0, 35.0}, {5.0, 70.0}, {11.0, 280.0}}, true);
    p.end_occasion();
  };
  for (int s = 0; s < 14; ++s) {
    occasion(s, s % 4 == 1, 10);
    if (s % 5 == 0) occasion(s, false, 10);
    p.end_subject();
  }
  for (int s = 14; s < 17; ++s) {  // another shape, too few for a class
    occasion(s, false, 4);
    p.end_subject();
  }
  for (int s = 17; s < 19; ++s) {  // steps 1, 2, 3, 3, 2, 1, 1, 2: a kept propagator is evicted for one needed sooner
    p.bolus(0.0, 100.0 + s);
    double time = 0.0;
    for (double dt : {1.0, 2.0, 3.0, 3.0, 2.0, 1.0, 1.0, 2.0}) p.obs(time += dt);
    p.cov({{0.0, 60.0 + s}, {30.0, 90.0 - s}});
    p.cov({{0.0, 140.0}}, true);
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// ODE: infusions on two inputs with shared and strictly-inside boundaries, boluses, several occasions
Pop pop_ode(uint64_t seed) {
  Pop p = pop_ragged(seed, 12);
  p.infusion(0.0, 100.0, 2.0);
  p.infusion(1.0, 50.0, 1.0, 1);  // ends where the first one ends
  p.infusion(3.0, 50.0, 0.0, 1);  // no duration: skipped
  p.bolus(0.5, 10.0);
  p.obs(0.25);
  p.obs(2.5);
  p.obs(2.5);
  p.obs(7.0);
  p.end_occasion();
  p.end_subject();
  return p;
}
Pop pop_ode_cov() {
  Pop p;
  p.n_cov = 1;
  for (int s = 0; s < 5; ++s) {
    p.infusion(0.0, 100.0 + s, 1.5);
    p.bolus(2.0, 10.0);
    for (int i = 1; i <= 5; ++i) p.obs(i * 1.25);
    p.cov({{s == 3 ? 2.0 : 0.0, 60.0 + s}, {4.0, 70.0}, {9.0, 65.0 - s}}, s == 4);  // (subject 3: ops before the first knot)
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// two subjects of 65 600 fused steps each: the class program does not fit the chunk header's 16-bit length
Pop pop_huge() {
  Pop p;
  p.presorted = true;
  for (int s = 0; s < 2; ++s) {
    p.bolus(0.0, 100.0 + s);
    for (int i = 1; i <= 65600; ++i) p.obs(i * 0.25);
    p.end_occasion();
    p.end_subject();
  }
  return p;
}

// ---- keys (every shape key_for can produce) -------------------------------------------------------------------------
pmx::CompileKey key_plain(int g, bool ladder = true) {
  pmx::CompileKey k;
  k.class_g = g;
  k.ladder = ladder;
  return k;
}
pmx::CompileKey key_lag(uint32_t mask, int g) {
  pmx::CompileKey k;
  k.lag_mask = mask;
  k.class_g = g;
  return k;
}
// derived 0 = theta * (size/70)^2 * (1 + 0.25 (wt - 70)); derived 1 = theta * (size/70)^-1
pmx::CompileKey key_dyn(int cov_time_mode) {
  pmx::CompileKey k;
  k.cov_time_mode = cov_time_mode;
  k.n_derived = 2;
  k.derived[0].src_param = 1;
  k.derived[0].n_factors = 2;
  k.derived[0].f[0] = {PMX_F_POW, 1, 70.0, 2.0};
  k.derived[0].f[1] = {PMX_F_LIN, 0, 70.0, 0.25};
  k.derived[1].src_param = 4;
  k.derived[1].n_factors = 1;
  k.derived[1].f[0] = {PMX_F_POW, 1, 70.0, -1.0};
  return k;
}
pmx::CompileKey key_dyn_classed(int cov_time_mode) {
  pmx::CompileKey k = key_dyn(cov_time_mode);
  k.class_g = 8;
  return k;
}
pmx::CompileKey key_dyn_cached(int cov_time_mode, int slots, bool kfac) {
  pmx::CompileKey k = key_dyn(cov_time_mode);
  k.prop_cache_slots = slots;
  if (kfac) {  // kernel parameters 1 and 4 are derived values, the rest primary
    k.kfac_n = 6;
    k.kfac_map[1] = 0;
    k.kfac_map[4] = 1;
  }
  return k;
}
pmx::CompileKey key_user_analytical(bool user_eq, bool user_lag, bool pm) {
  pmx::CompileKey k;
  k.rate_input = (pm && !user_eq) ? 1 : 0;
  k.full_rates = user_eq;
  k.n_rate = user_eq ? 2 : 1;
  k.want_times = true;
  k.solve_marks = true;
  k.user_cov = true;
  if (user_lag) {
    k.lag_merge = true;
    k.lag_mask = 3u;
  }
  return k;
}
pmx::CompileKey key_ode(int n_rate, bool want_times, uint32_t lag_mask) {
  pmx::CompileKey k;
  k.eq_kind = PMX_EQ_ODE;
  k.cov_time_mode = PMX_COV_TIME_SEGMENT_END_ABS;
  k.rk4_h_max = 0.125;
  k.n_rate = n_rate;
  k.want_times = want_times;
  k.lag_mask = lag_mask;
  return k;
}
pmx::CompileKey key_user_ode(bool user_lag) {
  pmx::CompileKey k = key_ode(2, true, 0);
  k.user_cov = true;
  if (user_lag) {
    k.lag_merge = true;
    k.lag_mask = 3u;
  }
  return k;
}

// ---- fingerprint ----------------------------------------------------------------------------------------------------
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ULL;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ULL;
  }
  template <class T>
  void pod(const T& v) {
    bytes(&v, sizeof(T));
  }
  void flag(bool v) {
    const unsigned char b = v ? 1 : 0;
    bytes(&b, 1);
  }
};

const char* g_case = "";
void line(const char* field, size_t n, const Fnv& f) { std::printf("%s %s %zu %016" PRIx64 "\n", g_case, field, n, f.h); }
template <class T>
void vec(const char* field, const std::vector<T>& v) {
  Fnv f;
  if (!v.empty()) f.bytes(v.data(), v.size() * sizeof(T));
  line(field, v.size(), f);
}
template <class T>
void scalar(const char* field, const T& v) {
  Fnv f;
  f.pod(v);
  line(field, 1, f);
}
void flag(const char* field, bool v) {
  Fnv f;
  f.flag(v);
  line(field, 1, f);
}
void key_line(const char* field, const pmx::CompileKey& k) {  // field by field: the struct has padding
  Fnv f;
  f.pod(k.eq_kind);
  f.pod(k.cov_time_mode);
  f.pod(k.rk4_h_max);
  f.pod(k.n_rate);
  f.pod(k.rate_input);
  f.pod(k.class_g);
  f.pod(k.lag_mask);
  f.pod(k.n_derived);
  for (const pmx_derived& d : k.derived) {
    f.pod(d.src_param);
    f.pod(d.n_factors);
    for (const pmx_factor& q : d.f) {
      f.pod(q.op);
      f.pod(q.cov);
      f.pod(q.ref);
      f.pod(q.coef);
    }
  }
  f.flag(k.want_times);
  f.flag(k.lag_merge);
  f.flag(k.solve_marks);
  f.flag(k.full_rates);
  f.flag(k.user_cov);
  f.pod(k.prop_cache_slots);
  f.pod(k.kfac_n);
  f.bytes(k.kfac_map, sizeof(k.kfac_map));
  f.flag(k.ladder);
  line(field, 1, f);
}

void fingerprint(const pmx::StreamPlan& sp) {
  const pmx::OpStream& os = sp.os;
  key_line("os.key", os.key);
  scalar("os.n_ops", os.n_ops);
  vec("os.subj_op_off", os.subj_op_off);
  vec("os.op_meta", os.op_meta);
  vec("os.op_a", os.op_a);
  vec("os.op_b", os.op_b);
  vec("os.op_n", os.op_n);
  vec("os.op_rate", os.op_rate);
  vec("os.op_cov", os.op_cov);
  vec("os.op_fac", os.op_fac);
  vec("os.op_t0", os.op_t0);
  vec("os.op_t1", os.op_t1);
  scalar("os.n_lag_slots", os.n_lag_slots);
  vec("os.lagb_off", os.lagb_off);
  vec("os.lagb_time", os.lagb_time);
  vec("os.lagb_amount", os.lagb_amount);
  vec("os.lagb_input", os.lagb_input);
  scalar("os.max_lagb_per_list", os.max_lagb_per_list);
  scalar("os.prop_cache_used", os.prop_cache_used);
  scalar("os.n_prop_reused", os.n_prop_reused);
  vec("os.subj_order", os.subj_order);
  scalar("os.max_ops_per_subject", os.max_ops_per_subject);
  scalar("os.n_prop", os.n_prop);
  scalar("os.max_input_used", os.max_input_used);
  vec("op_rec", sp.op_rec);
  vec("op_kfac", sp.op_kfac);
  vec("subj_step_off", sp.subj_step_off);
  vec("step_rec", sp.step_rec);
  const pmx::ClassPlan& cp = sp.cp;
  scalar("cp.G", cp.G);
  scalar("cp.n_chunks", cp.n_chunks);
  scalar("cp.n_classed_subjects", cp.n_classed_subjects);
  vec("cp.prog_meta", cp.prog_meta);
  vec("cp.prog_dt", cp.prog_dt);
  vec("cp.prog_t0", cp.prog_t0);
  vec("cp.prog_t1", cp.prog_t1);
  vec("cp.cls_prog_off", cp.cls_prog_off);
  vec("cp.cls_fast_mask", cp.cls_fast_mask);
  vec("cp.chunk_cls", cp.chunk_cls);
  vec("cp.chunk_n", cp.chunk_n);
  vec("cp.chunk_val_off", cp.chunk_val_off);
  vec("cp.chunk_subj", cp.chunk_subj);
  vec("cp.chunk_row", cp.chunk_row);
  vec("cp.val", cp.val);
  vec("cp.chunk_rate_mask", cp.chunk_rate_mask);
  scalar("cp.n_chunks_exact", cp.n_chunks_exact);
  vec("cp.dtv", cp.dtv);
  scalar("cp.n_fac", cp.n_fac);
  vec("cp.facp", cp.facp);
  vec("cp.faco", cp.faco);
  vec("cp.generic_subjects", cp.generic_subjects);
  vec("prog_rec", sp.prog_rec);
  vec("chunk_nobs", sp.chunk_nobs);
  vec("chunk_obs_off", sp.chunk_obs_off);
  scalar("cobs_size", sp.cobs_size);
  vec("chunk_hdr", sp.chunk_hdr);
  flag("no_rates", sp.no_rates);
  flag("eig_reuse", sp.eig_reuse);
  scalar("prop_reuse_fraction", sp.prop_reuse_fraction);
}

int g_failures = 0;
void run_case(const char* name, const Pop& pop, const pmx::CompileKey& key, const pmx::ClassTunables& ct = {}) {
  g_case = name;
  const pmx_population_desc d = pop.desc();
  pmx::HostPopulation hp;
  std::string err;
  int32_t rc = pmx::build_host_population(&d, &hp, &err);
  pmx::StreamPlan sp;
  if (rc == PMX_OK) rc = pmx::plan_stream(hp, key, ct, &sp, &err);
  scalar("rc", rc);
  if (rc != PMX_OK) {
    std::fprintf(stderr, "%s: %s\n", name, err.c_str());
    ++g_failures;
    return;
  }
  fingerprint(sp);
}

void corpus() {
  const Pop shared = pop_shared(), jitter = pop_jitter(), ragged = pop_ragged(3, 48), edges = pop_edges();
  const Pop long_prog = pop_long(), ladder = pop_ladder(), pm = pop_pm(), lag = pop_lag(), cov = pop_cov();
  const Pop ode = pop_ode(5), ode_cov = pop_ode_cov();
  // plain analytical
  run_case("shared_g8", shared, key_plain(8));
  run_case("shared_g4", shared, key_plain(4));
  run_case("shared_g8_packed", shared, key_plain(8), pmx::ClassTunables{0, 0, 0});  // no spread, no loose classes
  run_case("shared_noclass", shared, key_plain(0, false));
  run_case("jitter_g8", jitter, key_plain(8));
  run_case("jitter_g4", jitter, key_plain(4));
  run_case("jitter_g8_noloose", jitter, key_plain(8), pmx::ClassTunables{0, -1, 0});
  run_case("ragged_g8", ragged, key_plain(8));
  run_case("ragged_g4_min1", ragged, key_plain(4), pmx::ClassTunables{1, -1, -1});
  run_case("edges_g8", edges, key_plain(8));
  run_case("edges_g4_min1", edges, key_plain(4), pmx::ClassTunables{1, -1, -1});
  run_case("long_g8", long_prog, key_plain(8));
  run_case("ladder_g8", ladder, key_plain(8));
  run_case("ladder_g4_noladder", ladder, key_plain(4, false));
  run_case("huge_g4", pop_huge(), key_plain(4));
  // pm_ indexing
  {
    pmx::CompileKey k = key_plain(8);
    k.rate_input = 1;
    run_case("pm_g8", pm, k);
    run_case("ragged_pm_g8", ragged, k);
  }
  // lag
  run_case("lag_in0_g8", lag, key_lag(1u, 8));
  run_case("lag_in1_g4", lag, key_lag(2u, 4));
  run_case("lag_in0_in1", lag, key_lag(3u, 0));
  run_case("lag_in0_in1_g8", lag, key_lag(3u, 8));  // (a plan is asked for but two lagged inputs get none)
  run_case("ragged_lag_in1_g8", ragged, key_lag(2u, 8));
  // covariate-derived constants
  for (int mode : {PMX_COV_TIME_SEGMENT_DT, PMX_COV_TIME_SEGMENT_END_ABS}) {
    const std::string m = mode == PMX_COV_TIME_SEGMENT_DT ? "dt" : "abs";
    run_case(("cov_classed_" + m).c_str(), cov, key_dyn_classed(mode));
    for (int slots = 0; slots <= 3; ++slots) {
      run_case(("cov_cache" + std::to_string(slots) + "_" + m).c_str(), cov, key_dyn_cached(mode, slots, false));
      run_case(("cov_cache" + std::to_string(slots) + "_kfac_" + m).c_str(), cov, key_dyn_cached(mode, slots, true));
    }
  }
  {
    pmx::CompileKey k;  // covariates without derived values: op_cov only
    run_case("cov_plain", cov, k);
  }
  // user (run-time compiled) analytical models
  run_case("user_an", ragged, key_user_analytical(false, false, false));
  run_case("user_an_pm", pm, key_user_analytical(false, false, true));
  run_case("user_an_eq", edges, key_user_analytical(true, false, false));
  run_case("user_an_eq_lag", lag, key_user_analytical(true, true, false));
  run_case("user_an_lag_ragged", ragged, key_user_analytical(false, true, false));
  run_case("user_an_cov", cov, key_user_analytical(true, false, false));
  // ODE
  run_case("ode_r1", ode, key_ode(1, false, 0));
  run_case("ode_r2", ode, key_ode(2, false, 0));
  run_case("ode_r2_times", ode, key_ode(2, true, 0));
  run_case("ode_edges_r1_times", edges, key_ode(1, true, 0));
  run_case("ode_lag_in0", lag, key_ode(3, false, 1u));
  run_case("ode_lag_in0_in1", lag, key_ode(3, true, 3u));
  run_case("ode_cov", ode_cov, key_ode(1, false, 0));
  run_case("ode_user", ode, key_user_ode(false));
  run_case("ode_user_lag", lag, key_user_ode(true));
  run_case("ode_user_cov", ode_cov, key_user_ode(true));
}

// ---- timing -----------------------------------------------------------------------------------------------------------
void time_case(const char* name, const Pop& pop, const pmx::CompileKey& key, int n) {
  const pmx_population_desc d = pop.desc();
  pmx::HostPopulation hp;
  std::string err;
  if (pmx::build_host_population(&d, &hp, &err) != PMX_OK) {
    std::fprintf(stderr, "%s: %s\n", name, err.c_str());
    ++g_failures;
    return;
  }
  std::vector<double> ms;
  int64_t sink = 0;
  for (int i = 0; i < n; ++i) {
    pmx::StreamPlan sp;
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = pmx::plan_stream(hp, key, pmx::ClassTunables{}, &sp, &err);
    const auto t1 = std::chrono::steady_clock::now();
    if (rc != PMX_OK) ++g_failures;
    sink += sp.os.n_ops + sp.cp.n_chunks;
    ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  std::printf("%s subjects=%" PRId64 " runs=%d best_ms=%.3f median_ms=%.3f (ops+chunks=%" PRId64 ")\n", name, hp.n_subjects, n, ms.front(),
              ms[ms.size() / 2], sink / n);
}

void timing(int n) {
  {  // C3 shape: one protocol, infusion + 7 observations = 15 ops per subject, two-compartment key
    Pop p;
    Rng rng(3);
    add_design(&p, 100000, &rng, false);
    time_case("c3_plain_g8", p, key_plain(8), n);
  }
  {  // C5 shape: three oral doses + 10 observations, a weight covariate of 2..4 knots, k10 = k10_0 (wt/70)^0.75
    Pop p;
    p.n_cov = 1;
    Rng rng(5);
    const double obs_t[10] = {1.0, 2.0, 4.0, 8.0, 12.0, 23.5, 26.0, 36.0, 50.0, 72.0};
    for (int s = 0; s < 20000; ++s) {
      const double amt = 100.0 + 400.0 * rng.unit();
      for (int j = 0; j < 3; ++j) p.bolus(24.0 * j, amt);
      for (double t : obs_t) p.obs(t);
      const int nk = 2 + rng.below(3);
      for (int k = 0; k < nk; ++k) {
        p.kt.push_back(k == 0 ? 0.0 : (k + rng.unit() * 0.9) * 18.0);
        p.kv.push_back(50.0 + 60.0 * rng.unit());
      }
      p.knot_off.push_back(static_cast<int64_t>(p.kt.size()));
      p.fixed.push_back(0);
      p.end_occasion();
      p.end_subject();
    }
    pmx::CompileKey k;
    k.n_derived = 1;
    k.derived[0].src_param = 1;
    k.derived[0].n_factors = 1;
    k.derived[0].f[0] = {PMX_F_POW, 0, 70.0, 0.75};
    k.prop_cache_slots = 2;
    k.kfac_n = 6;
    k.kfac_map[1] = 0;
    time_case("c5_cov_cache2", p, k, n);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--time") == 0) {
    timing(std::max(1, std::atoi(argv[2])));
  } else if (argc == 1) {
    corpus();
  } else {
    std::fprintf(stderr, "usage: %s [--time N]\n", argv[0]);
    return 2;
  }
  return g_failures ? 1 : 0;
}

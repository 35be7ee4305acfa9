// pmx_plan.cpp — from an op stream to what goes on the device: the step stream, the class plan, the packed records and
// plan_stream, which runs them all (see pmx_compile.hpp).  Host C++ only (no HIP).
#include "pmx_compile.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>

namespace pmx {

namespace {

inline uint64_t mix64(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ULL + (h << 6) + (h >> 2);
  h *= 0xBF58476D1CE4E5B9ULL;
  return h ^ (h >> 31);
}
inline uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}
inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// what a fused observation adds to the step in front of it (or to an OP_OBS step of its own)
inline uint32_t obs_after(uint32_t outeq) { return (1u << kOpObsAfterShift) | ((outeq & kOpOutMask) << kOpOutShift); }
inline bool has_obs_after(uint32_t meta) { return ((meta >> kOpObsAfterShift) & 1u) != 0u; }

}  // namespace

void build_step_stream(const OpStream& os, std::vector<int64_t>* subj_step_off, std::vector<double>* rec) {
  const int64_t S = static_cast<int64_t>(os.subj_op_off.size()) - 1;
  subj_step_off->assign(static_cast<size_t>(S) + 1, 0);
  rec->clear();
  rec->reserve(static_cast<size_t>(os.n_ops) * 2 + 4);
  auto push = [&](uint64_t meta, double a, double b) {
    double w;
    std::memcpy(&w, &meta, 8);
    rec->push_back(w);
    rec->push_back(a);
    rec->push_back(b);
    rec->push_back(0.0);
  };
  int64_t n_steps = 0;
  for (int64_t s = 0; s < S; ++s) {
    int64_t last = -1;  // this subject's last step, if it can still take an observation
    for (int64_t o = os.subj_op_off[s]; o < os.subj_op_off[s + 1]; ++o) {
      const uint32_t meta = os.op_meta[o];
      if (op_kind(meta) == OP_OBS) {
        const uint64_t tag = obs_after(op_io(meta));
        if (last >= 0) {
          uint64_t w;
          std::memcpy(&w, &(*rec)[static_cast<size_t>(last) * 4], 8);
          w |= tag;
          std::memcpy(&(*rec)[static_cast<size_t>(last) * 4], &w, 8);
          last = -1;
        } else {
          push(static_cast<uint64_t>(OP_OBS) | tag, 0.0, 0.0);
          ++n_steps;
        }
      } else {  // kind | io | the PROP's ladder rung
        push(make_meta(op_kind(meta), op_io(meta)) | (meta & (kOpRungMask << kOpRungShift)), os.op_a[o], os.op_b[o]);
        last = n_steps++;
      }
    }
    (*subj_step_off)[static_cast<size_t>(s) + 1] = n_steps;
  }
  push(static_cast<uint64_t>(OP_OBS), 0.0, 0.0);  // padding: the walker requests one record past a subject's last step
}

uint32_t ladder_code(double dt, double* prev, double* span) {
  uint32_t code = 0;
  if (*prev > 0.0 && dt > 0.0) {
    for (uint32_t n = 1; n <= 4; ++n) {
      if (std::fabs(dt - n * *prev) <= 8.0 * std::numeric_limits<double>::epsilon() * dt && *span * n <= 1024.0) {
        code = n;
        break;
      }
    }
  }
  if (code) {
    *span *= code;
    *prev = code * *prev;
  } else {
    *span = 1.0;
    *prev = dt;
  }
  return code;
}

// ------------------------------------------------------------------------------------
// class plan
// ------------------------------------------------------------------------------------
namespace {

struct Classes {
  std::vector<int32_t> rep;                   // class -> representative = its first subject
  std::vector<std::vector<int32_t>> members;  // class -> subjects, in the order given
};

// Groups `subjects`: a subject joins the class whose representative it `same`s, else it founds the next class - so
// class ids follow the order of `subjects`, which the plan's byte layout depends on.
template <class Hash, class Same>
Classes group_subjects(const std::vector<int32_t>& subjects, Hash hash, Same same) {
  Classes g;
  std::unordered_map<uint64_t, std::vector<int32_t>> buckets;  // hash -> class ids
  for (int32_t s : subjects) {
    auto& ids = buckets[hash(s)];
    int32_t cls = -1;
    for (int32_t c : ids)
      if (same(g.rep[c], s)) {
        cls = c;
        break;
      }
    if (cls < 0) {
      cls = static_cast<int32_t>(g.rep.size());
      g.rep.push_back(s);
      g.members.emplace_back();
      ids.push_back(cls);
    }
    g.members[cls].push_back(s);
  }
  return g;
}

// Exact classes: members share op kinds, inputs, outeqs, every flag of the op word and the PROP lengths (BOLUS amount /
// PROP rate / OBS time are free).  Members of a lag class also share every absolute time a lane's lagged boluses are
// compared with: PROP [t0, t1), the first event's time of a RESET and the recorded times of the occasion's boluses.
uint64_t program_hash(const OpStream& os, bool lagged, int64_t s) {
  const int64_t o0 = os.subj_op_off[s], o1 = os.subj_op_off[s + 1];
  uint64_t h = static_cast<uint64_t>(o1 - o0);
  for (int64_t o = o0; o < o1; ++o) {
    const uint32_t kind = op_kind(os.op_meta[o]);
    const uint64_t bits = kind == OP_PROP ? bits_of(os.op_a[o]) : 0;
    h = mix64(h, (static_cast<uint64_t>(os.op_meta[o]) << 1) ^ (bits * 0x9E3779B97F4A7C15ULL) ^ bits);
    if (!lagged) continue;
    h = mix64(h, bits_of(os.op_t0[o]));
    if (kind == OP_RESET) {
      const int64_t oc = static_cast<int64_t>(os.op_a[o]);
      for (int64_t q = os.lagb_off[oc]; q < os.lagb_off[oc + 1]; ++q) h = mix64(h, bits_of(os.lagb_time[q]));
    }
  }
  return h;
}
bool same_program(const OpStream& os, bool lagged, int64_t a, int64_t b) {
  const int64_t a0 = os.subj_op_off[a], b0 = os.subj_op_off[b], n = os.subj_op_off[a + 1] - a0;
  if (n != os.subj_op_off[b + 1] - b0) return false;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t x = a0 + i, y = b0 + i;
    if (os.op_meta[x] != os.op_meta[y]) return false;
    const uint32_t kind = op_kind(os.op_meta[x]);
    if (kind == OP_PROP && !same_bits(os.op_a[x], os.op_a[y])) return false;
    if (!lagged) continue;
    if (kind == OP_PROP && !(same_bits(os.op_t0[x], os.op_t0[y]) && same_bits(os.op_t1[x], os.op_t1[y]))) return false;
    if (kind == OP_RESET) {
      if (!same_bits(os.op_t0[x], os.op_t0[y])) return false;
      const int64_t oa = static_cast<int64_t>(os.op_a[x]), ob = static_cast<int64_t>(os.op_a[y]);
      const int64_t la = os.lagb_off[oa], lb = os.lagb_off[ob], na = os.lagb_off[oa + 1] - la;
      if (na != os.lagb_off[ob + 1] - lb) return false;
      if (na > 0 && std::memcmp(&os.lagb_time[la], &os.lagb_time[lb], static_cast<size_t>(na) * 8) != 0) return false;
    }
  }
  return true;
}

// Loose classes share kind | io of every op; ladder bits and lengths are free.
constexpr uint32_t kShape = kOpKindMask | (kOpIoMask << kOpIoShift);
uint64_t shape_hash(const OpStream& os, int64_t s) {
  const int64_t o0 = os.subj_op_off[s], o1 = os.subj_op_off[s + 1];
  uint64_t h = static_cast<uint64_t>(o1 - o0);
  for (int64_t o = o0; o < o1; ++o) h = mix64(h, static_cast<uint64_t>(os.op_meta[o] & kShape));
  return h;
}
bool same_shape(const OpStream& os, int64_t x, int64_t y) {
  const int64_t x0 = os.subj_op_off[x], y0 = os.subj_op_off[y], n = os.subj_op_off[x + 1] - x0;
  if (n != os.subj_op_off[y + 1] - y0) return false;
  for (int64_t i = 0; i < n; ++i)
    if ((os.op_meta[x0 + i] & kShape) != (os.op_meta[y0 + i] & kShape)) return false;
  return true;
}

// pm_ indexing: a bolus into input 0 lands in the wrapper's pad slot (generic walker only)
bool doses_into_pad(const OpStream& os, int64_t s) {
  for (int64_t o = os.subj_op_off[s]; o < os.subj_op_off[s + 1]; ++o)
    if (op_kind(os.op_meta[o]) == OP_BOLUS && op_io(os.op_meta[o]) == 0u) return true;
  return false;
}

// A class's program, built from its representative.  Every OBS op is FUSED into the step before it (ObsAfter + Out), so
// a PROP+OBS pair costs one trip of the device loop; a second observation at the same instant gets a step of its own
// (kind OP_OBS = no state change).
struct ClassProgram {
  std::vector<int32_t> step_of_op;      // op (relative to the subject's first) -> its step, -1: an OBS op
  std::vector<int32_t> obs_step_of_op;  // OBS op -> the step that emits its row, -1: not an OBS op
  std::vector<uint32_t> meta;
  std::vector<double> dt, t0, t1;
  int64_t n_ops() const { return static_cast<int64_t>(step_of_op.size()); }
  int64_t n_steps() const { return static_cast<int64_t>(meta.size()); }
};

ClassProgram build_program(const OpStream& os, int32_t rep, bool lagged, bool ladder) {
  const int64_t r0 = os.subj_op_off[rep], n = os.subj_op_off[rep + 1] - r0;
  ClassProgram p;
  p.step_of_op.assign(static_cast<size_t>(n), -1);
  p.obs_step_of_op.assign(static_cast<size_t>(n), -1);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t o = r0 + i;
    const uint32_t kind = op_kind(os.op_meta[o]);
    if (kind == OP_OBS) {
      // Flush (lag models): lagged boluses may land in front of the observation; its time goes into the step's t1 slot,
      // which is free (the step is never a PROP)
      const uint32_t flush = os.op_meta[o] & (1u << kOpFlushShift);
      if (p.meta.empty() || has_obs_after(p.meta.back())) {
        p.meta.push_back(make_meta(OP_OBS, 0));
        p.dt.push_back(0.0);
        p.t0.push_back(0.0);
        p.t1.push_back(0.0);
      }
      p.meta.back() |= obs_after(op_io(os.op_meta[o])) | flush;
      if (flush) p.t1.back() = os.op_a[o];
      p.obs_step_of_op[i] = static_cast<int32_t>(p.meta.size()) - 1;
    } else {
      p.meta.push_back(make_meta(kind, op_io(os.op_meta[o])));
      p.dt.push_back(kind == OP_PROP ? os.op_a[o] : 0.0);
      p.t0.push_back(lagged ? os.op_t0[o] : 0.0);
      p.t1.push_back(lagged ? os.op_t1[o] : 0.0);
      p.step_of_op[i] = static_cast<int32_t>(p.meta.size()) - 1;
    }
  }
  if (ladder) {
    // Exponential ladder (pmx_structures.hpp ladder_pow): Rung of a PROP step = n when its length is n x the previous
    // PROP's (n = 1: same propagator again).  `span` = how many times the first rung's rounding error has been
    // multiplied; past 1024 the next step starts a fresh ladder.
    double prev = 0.0, span = 1.0;
    for (size_t i = 0; i < p.meta.size(); ++i)
      if (op_kind(p.meta[i]) == OP_PROP) p.meta[i] |= ladder_code(p.dt[i], &prev, &span) << kOpRungShift;
  }
  return p;
}

// ClassPlan::cls_fast_mask: PROP steps on the ladder (rung 1..4) with an observation of output 0 fused in, no Flush
uint64_t fast_mask(const ClassProgram& p) {
  uint64_t fast = 0;
  for (int64_t i = 0; i < p.n_steps() && i < 63; ++i) {
    const uint32_t sm = p.meta[i];
    const bool obs0 = has_obs_after(sm) && ((sm >> kOpOutShift) & kOpOutMask) == 0u;
    const uint32_t rung = (sm >> kOpRungShift) & kOpRungMask;
    if (op_kind(sm) == OP_PROP && obs0 && rung >= 1u && rung <= 4u && (sm >> kOpFlushShift) == 0u) fast |= 1ull << i;
  }
  return fast;
}

struct ClassPlanBuilder {
  const HostPopulation& hp;
  const OpStream& os;
  ClassPlan* cp;
  const int32_t G;
  const bool ladder, spread;
  const bool lagged;  // one lagged input (the caller only asks for a plan of a lag model then)
  const bool dyn;     // covariate-derived constants: nothing to share but the program shape
  const size_t nfac;

  // one class -> its program and its chunks; `loose`: the members' PROP lengths differ (dtv), no ladder
  void emit_class(const std::vector<int32_t>& mem, int32_t rep, bool loose) {
    const ClassProgram p = build_program(os, rep, lagged, ladder && !loose);
    const int32_t cls = static_cast<int32_t>(cp->cls_fast_mask.size());
    cp->prog_meta.insert(cp->prog_meta.end(), p.meta.begin(), p.meta.end());
    if (loose)
      cp->prog_dt.insert(cp->prog_dt.end(), p.dt.size(), 0.0);
    else
      cp->prog_dt.insert(cp->prog_dt.end(), p.dt.begin(), p.dt.end());
    cp->prog_t0.insert(cp->prog_t0.end(), p.t0.begin(), p.t0.end());
    cp->prog_t1.insert(cp->prog_t1.end(), p.t1.begin(), p.t1.end());
    cp->cls_prog_off.push_back(static_cast<int64_t>(cp->prog_meta.size()));
    cp->cls_fast_mask.push_back(fast_mask(p));
    // Which members share a chunk is free (any G subjects of the class may share a propagator).  `spread`: member j of
    // chunk c is the (c + j * n_chunks)-th subject of the class, so the G rows a block writes at one step are far
    // apart while neighbouring blocks write neighbouring subjects: G slowly advancing write fronts instead of every
    // block covering its own 8-subject region (tools/experiments/store_pattern_probe.hip, rows B vs H).
    const size_t n_chunks = (mem.size() + static_cast<size_t>(G) - 1) / static_cast<size_t>(G);
    std::vector<int32_t> pick(static_cast<size_t>(G));
    for (size_t c = 0; c < n_chunks; ++c) {
      int32_t n = 0;
      for (int32_t j = 0; j < G; ++j) {
        const size_t idx = spread ? (c + static_cast<size_t>(j) * n_chunks) : (c * static_cast<size_t>(G) + static_cast<size_t>(j));
        if (idx < mem.size()) pick[n++] = mem[idx];
      }
      fill_chunk(p, cls, pick.data(), n, loose);
    }
  }

  // one chunk: its `n` members' ids and rows, their per-step values (val, dtv, facp, faco) and the rate mask
  void fill_chunk(const ClassProgram& p, int32_t cls, const int32_t* pick, int32_t n, bool loose) {
    const int64_t L = p.n_steps();
    cp->chunk_cls.push_back(cls);
    cp->chunk_n.push_back(n);
    cp->chunk_val_off.push_back(static_cast<int64_t>(cp->val.size()));
    for (int32_t j = 0; j < G; ++j) {
      cp->chunk_subj.push_back(j < n ? pick[j] : -1);
      cp->chunk_row.push_back(j < n ? hp.subj_obs_off[pick[j]] : 0);
    }
    const size_t base = cp->val.size(), end = base + static_cast<size_t>(L) * G;
    cp->val.resize(end, 0.0);
    cp->dtv.resize(end, 0.0);
    if (dyn) {
      cp->facp.resize(end * nfac, 1.0);
      cp->faco.resize(end * nfac, 1.0);
    }
    auto at = [&](int32_t step, int32_t j) { return base + static_cast<size_t>(step) * G + j; };
    for (int32_t j = 0; j < n; ++j) {
      const int64_t s0 = os.subj_op_off[pick[j]];
      for (int64_t i = 0; i < p.n_ops(); ++i) {
        const int32_t st = p.step_of_op[i], so = p.obs_step_of_op[i];
        const uint32_t kind = op_kind(os.op_meta[s0 + i]);
        if (dyn) {  // this member's covariate factors at the op: the PROP's rate constants, the observation's volume
          const double* src = &os.op_fac[static_cast<size_t>(s0 + i) * nfac];
          if (so >= 0)
            std::memcpy(&cp->faco[at(so, j) * nfac], src, nfac * sizeof(double));
          else if (st >= 0 && kind == OP_PROP)
            std::memcpy(&cp->facp[at(st, j) * nfac], src, nfac * sizeof(double));
        }
        if (st < 0) continue;
        double v = 0.0;
        if (kind == OP_BOLUS) v = os.op_a[s0 + i];
        if (kind == OP_PROP) v = os.op_b[s0 + i];
        if (kind == OP_RESET && lagged) v = os.op_a[s0 + i];  // this member's occasion: where its lagged boluses are listed
        cp->val[at(st, j)] = v;
        if (loose && kind == OP_PROP) cp->dtv[at(st, j)] = os.op_a[s0 + i];
      }
    }
    uint64_t mask = 0;
    for (int64_t st = 0; st < L; ++st) {
      bool any = false;
      for (int32_t j = 0; j < n; ++j) any |= cp->val[at(static_cast<int32_t>(st), j)] != 0.0;
      if (any) mask |= 1ull << (st < 63 ? st : 63);
    }
    if (L > 63) mask |= 1ull << 63;  // (steps past the mask's width always fetch their values)
    cp->chunk_rate_mask.push_back(mask);
    cp->n_classed_subjects += n;
  }
};

}  // namespace

void build_class_plan(const HostPopulation& hp, const OpStream& os, int32_t G, int32_t min_class_size, ClassPlan* cp,
                      bool ladder, bool spread, bool loose_classes) {
  *cp = ClassPlan{};
  cp->G = G;
  const size_t nfac = static_cast<size_t>(os.key.n_derived) * PMX_MAX_FACTORS;
  cp->n_fac = static_cast<int32_t>(nfac);
  if (os.n_lag_slots > 1) return;
  const bool dyn = os.key.n_derived > 0 && !os.op_fac.empty(), lagged = os.n_lag_slots == 1;
  if (dyn) loose_classes = true;
  if (lagged) loose_classes = false;  // loose members do not share the times
  ClassPlanBuilder b{hp, os, cp, G, ladder, spread, lagged, dyn, nfac};

  std::vector<int32_t> candidates;
  for (int64_t s = 0; s < hp.n_subjects; ++s) {
    // an empty subject: nothing to compute, but the generic walker still owns its status bytes
    // ... and so does one that never propagates: the classed kernels fail every member of a lane with complex eigenvalues,
    // which is the walkers' rule (fail at the first PROP) only for programs that have one
    bool propagates = false;
    for (int64_t o = os.subj_op_off[s]; o < os.subj_op_off[s + 1] && !propagates; ++o) propagates = op_kind(os.op_meta[o]) == OP_PROP;
    const bool generic = !propagates || (os.key.rate_input == 1 && doses_into_pad(os, s));
    (generic ? cp->generic_subjects : candidates).push_back(static_cast<int32_t>(s));
  }
  const Classes exact = group_subjects(
      candidates, [&](int32_t s) { return program_hash(os, lagged, s); },
      [&](int32_t a, int32_t s) { return same_program(os, lagged, a, s); });
  cp->cls_prog_off.push_back(0);
  std::vector<int32_t> leftover;  // members of classes too small to batch: second chance as loose classes
  for (size_t c = 0; c < exact.members.size(); ++c) {
    if (dyn || static_cast<int32_t>(exact.members[c].size()) < min_class_size)
      leftover.insert(leftover.end(), exact.members[c].begin(), exact.members[c].end());
    else
      b.emit_class(exact.members[c], exact.rep[c], false);
  }
  cp->n_chunks_exact = static_cast<int64_t>(cp->chunk_cls.size());
  if (loose_classes && !leftover.empty()) {
    std::sort(leftover.begin(), leftover.end());
    const Classes loose = group_subjects(
        leftover, [&](int32_t s) { return shape_hash(os, s); }, [&](int32_t a, int32_t s) { return same_shape(os, a, s); });
    // a loose chunk does G members' arithmetic whatever it holds (no propagator to share): below ~3/4 full the
    // generic walker is the cheaper way to serve its subjects
    const int32_t min_loose = std::max(min_class_size, (3 * G + 3) / 4);
    for (size_t c = 0; c < loose.members.size(); ++c) {
      if (static_cast<int32_t>(loose.members[c].size()) < min_loose)
        cp->generic_subjects.insert(cp->generic_subjects.end(), loose.members[c].begin(), loose.members[c].end());
      else
        b.emit_class(loose.members[c], loose.rep[c], true);
    }
  } else {
    cp->generic_subjects.insert(cp->generic_subjects.end(), leftover.begin(), leftover.end());
  }
  cp->n_chunks = static_cast<int64_t>(cp->chunk_cls.size());
  cp->chunk_val_off.push_back(static_cast<int64_t>(cp->val.size()));  // sentinel: chunk c's block is [off[c], off[c+1])
  std::sort(cp->generic_subjects.begin(), cp->generic_subjects.end());
}

// ------------------------------------------------------------------------------------
// packed records, plan_stream
// ------------------------------------------------------------------------------------
namespace {

// packed per-op records (pmx_devtypes.hpp DevOps::op_rec): ODE [6] = {meta | n << 32 (bits), a, b, rate[0], t0, t1},
// analytical [4] = {meta (bits), a, b, t0}
void pack_op_rec(const OpStream& os, const CompileKey& key, std::vector<double>* out) {
  const bool times = !os.op_t0.empty(), ode = key.eq_kind == PMX_EQ_ODE;
  const size_t w = ode ? 6 : 4;
  std::vector<double> rec(static_cast<size_t>(os.n_ops) * w, 0.0);
  for (int64_t o = 0; o < os.n_ops; ++o) {
    double* r = &rec[w * static_cast<size_t>(o)];
    const uint64_t m = os.op_meta[o] | (ode ? static_cast<uint64_t>(static_cast<uint32_t>(os.op_n[o])) << 32 : 0);
    std::memcpy(r, &m, 8);
    r[1] = os.op_a[o];
    r[2] = os.op_b[o];
    if (ode) r[3] = key.n_rate > 0 ? os.op_rate[o * key.n_rate] : 0.0;
    r[ode ? 4 : 3] = times ? os.op_t0[o] : 0.0;
    if (ode) r[5] = times ? os.op_t1[o] : 0.0;
  }
  out->swap(rec);
}

// one 64-byte record per op for the matrix-free walker (DevOps::op_kfac)
void pack_op_kfac(const OpStream& os, const CompileKey& key, std::vector<double>* out) {
  const size_t n_ops = os.op_meta.size();
  const size_t fw = static_cast<size_t>(key.n_derived) * PMX_MAX_FACTORS;
  std::vector<double> kf(n_ops * 8, 1.0);
  for (size_t o = 0; o < n_ops; ++o) {
    for (int j = 0; j < key.kfac_n && j < 7; ++j) {
      const int dd = key.kfac_map[j];
      if (dd < 0 || dd >= key.n_derived) continue;
      double f = 1.0;  // the parameter's factors multiplied out: theta * (f0 * f1) for the descriptor's (theta * f0) * f1
      for (int q = 0; q < key.derived[dd].n_factors && q < PMX_MAX_FACTORS; ++q) f *= os.op_fac[o * fw + static_cast<size_t>(dd) * PMX_MAX_FACTORS + q];
      kf[o * 8 + j] = f;
    }
    kf[o * 8 + 7] = os.op_a[o];
  }
  out->swap(kf);
}

// One 64-byte record per chunk for pmx_analytical_classed_ll (pmx_kernels.hpp DevClassPlan::chunk_hdr): everything the
// kernel needs of a chunk in ONE scalar fetch.  32-bit offsets and 16-bit counts: a plan outside those limits simply
// keeps the round-2 kernel (chunk_hdr stays empty).
void pack_chunk_hdr(StreamPlan* sp) {
  const ClassPlan& cp = sp->cp;
  constexpr int64_t k32 = int64_t{1} << 32;
  bool fits = cp.G <= 8 && sp->cobs_size < k32 && static_cast<int64_t>(cp.val.size()) < k32 &&
              static_cast<int64_t>(cp.prog_meta.size()) < k32;
  for (size_t cl = 0; cl + 1 < cp.cls_prog_off.size() && fits; ++cl)
    fits = cp.cls_prog_off[cl + 1] - cp.cls_prog_off[cl] < 65536;
  if (!fits) return;
  std::vector<uint32_t> hdr((static_cast<size_t>(cp.n_chunks) + 1) * 16, 0);
  for (int64_t c = 0; c < cp.n_chunks; ++c) {
    uint32_t* q = &hdr[static_cast<size_t>(c) * 16];
    const int32_t cl = cp.chunk_cls[c];
    q[0] = static_cast<uint32_t>(cp.chunk_n[c]) | (static_cast<uint32_t>(cp.cls_prog_off[cl + 1] - cp.cls_prog_off[cl]) << 16);
    q[1] = static_cast<uint32_t>(cp.cls_prog_off[cl]);
    q[2] = static_cast<uint32_t>(cp.chunk_val_off[c]);
    q[3] = static_cast<uint32_t>(sp->chunk_obs_off[c]);
    const uint64_t rm = cp.chunk_rate_mask[c], fm = cp.cls_fast_mask[cl];
    q[4] = static_cast<uint32_t>(rm);
    q[5] = static_cast<uint32_t>(rm >> 32);
    q[6] = static_cast<uint32_t>(fm);
    q[7] = static_cast<uint32_t>(fm >> 32);
    for (int32_t j = 0; j < cp.G; ++j) q[8 + j] = static_cast<uint32_t>(cp.chunk_subj[static_cast<size_t>(c) * cp.G + j]);
  }
  sp->chunk_hdr.swap(hdr);
}

// what the log-likelihood kernels read of a class plan besides the plan itself: prog_rec, the per-chunk observation
// counts and block offsets, and the chunk headers
void pack_class_ll(StreamPlan* sp) {
  const ClassPlan& cp = sp->cp;
  std::vector<double> prec((cp.prog_meta.size() + 1) * 2, 0.0);
  for (size_t i = 0; i < cp.prog_meta.size(); ++i) {
    const uint64_t w = cp.prog_meta[i];
    std::memcpy(&prec[2 * i], &w, 8);
    prec[2 * i + 1] = cp.prog_dt[i];
  }
  sp->prog_rec.swap(prec);
  sp->chunk_nobs.resize(static_cast<size_t>(cp.n_chunks));
  sp->chunk_obs_off.resize(static_cast<size_t>(cp.n_chunks) + 1);
  int64_t at = 0;
  for (int64_t c = 0; c < cp.n_chunks; ++c) {
    const int32_t cl = cp.chunk_cls[c];
    int32_t nobs = 0;
    for (int64_t o = cp.cls_prog_off[cl]; o < cp.cls_prog_off[cl + 1]; ++o) nobs += has_obs_after(cp.prog_meta[o]);
    sp->chunk_nobs[c] = nobs;
    sp->chunk_obs_off[c] = at;
    at += (static_cast<int64_t>(nobs) * 2 + 2) * cp.G;
  }
  sp->chunk_obs_off[cp.n_chunks] = at;  // sentinel
  sp->cobs_size = at;
  pack_chunk_hdr(sp);
}

}  // namespace

int32_t plan_stream(const HostPopulation& hp, const CompileKey& key, const ClassTunables& ct, StreamPlan* sp, std::string* err) {
  OpStream& os = sp->os;
  const int32_t rc = compile_ops(hp, key, &os, err);
  if (rc != PMX_OK) return rc;
  pack_op_rec(os, key, &sp->op_rec);
  if (key.kfac_n > 0 && !os.op_fac.empty()) pack_op_kfac(os, key, &sp->op_kfac);
  sp->no_rates = true;  // (analytical streams: a PROP's op_b is its rate)
  for (size_t o = 0; o < os.op_meta.size() && sp->no_rates; ++o)
    if (op_kind(os.op_meta[o]) == OP_PROP && os.op_b[o] != 0.0) sp->no_rates = false;
  sp->eig_reuse = false;  // (covariate streams: SameFac on some PROP)
  if (key.prop_cache_slots > 0 && !os.op_fac.empty())
    for (size_t o = 0; o < os.op_meta.size() && !sp->eig_reuse; ++o)
      if (op_kind(os.op_meta[o]) == OP_PROP && (os.op_meta[o] & kOpSameFacBit)) sp->eig_reuse = true;
  sp->prop_reuse_fraction = os.n_prop > 0 ? static_cast<double>(os.n_prop_reused) / static_cast<double>(os.n_prop) : 0.0;
  if (key.eq_kind == PMX_EQ_ANALYTICAL && !key.user_cov && key.lag_mask == 0 && os.op_fac.empty())
    build_step_stream(os, &sp->subj_step_off, &sp->step_rec);
  if (key.class_g > 0) {
    const int32_t min_class = ct.min_class > 0 ? ct.min_class : key.class_g / 2;
    const bool spread = ct.spread < 0 ? true : ct.spread != 0;  // (0.94-0.97 vs 1.05-1.11 ms on C3 in most allocations, never slower: tools/experiments/alloc_tune.py)
    const bool loose = ct.loose < 0 ? true : ct.loose != 0;  // subjects without a shared design still share a program shape: batched with per-member step lengths
    build_class_plan(hp, os, key.class_g, min_class, &sp->cp, key.ladder, spread, loose);
    if (sp->cp.n_chunks > 0) pack_class_ll(sp);
  }
  return PMX_OK;
}

}  // namespace pmx

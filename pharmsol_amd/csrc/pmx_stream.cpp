// pmx_stream.cpp — the device side of a (population, model flavour) pair: plan on the host (pmx_compile.cpp
// plan_stream), upload, and the log-likelihood's sigma-table slots.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "pmx_internal.hpp"

namespace {

template <class T>
int32_t upload(const std::vector<T>& v, const T** out, std::vector<void*>* allocs) {
  *out = nullptr;
  if (v.empty()) return PMX_OK;
  void* p = nullptr;
  PMX_HIP(hipMalloc(&p, v.size() * sizeof(T)));
  allocs->push_back(p);
  PMX_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = static_cast<const T*>(p);
  return PMX_OK;
}

// uploads in sequence; after a failure the rest are skipped and rc holds the first error
struct Uploader {
  std::vector<void*>* allocs;
  int32_t rc = PMX_OK;
  template <class T>
  void operator()(const std::vector<T>& v, const T** out) {
    if (rc == PMX_OK) rc = upload(v, out, allocs);
  }
};

void upload_class_plan(const pmx::StreamPlan& sp, DeviceStream* ds, Uploader& up) {
  const pmx::ClassPlan& cp = sp.cp;
  pmx::DevClassPlan& c = ds->cls;
  up(cp.prog_meta, &c.prog_meta);
  up(cp.prog_dt, &c.prog_dt);
  up(sp.prog_rec, &c.prog_rec);
  up(cp.chunk_rate_mask, &c.chunk_rate_mask);
  up(cp.cls_fast_mask, &c.cls_fast_mask);
  up(cp.prog_t0, &c.prog_t0);
  up(cp.prog_t1, &c.prog_t1);
  up(cp.cls_prog_off, &c.cls_prog_off);
  up(cp.chunk_cls, &c.chunk_cls);
  up(cp.chunk_n, &c.chunk_n);
  up(cp.chunk_val_off, &c.chunk_val_off);
  up(cp.chunk_subj, &c.chunk_subj);
  up(cp.chunk_row, &c.chunk_row);
  up(cp.val, &c.val);
  up(cp.dtv, &c.dtv);
  up(cp.facp, &c.facp);
  up(cp.faco, &c.faco);
  up(cp.generic_subjects, &c.generic_subjects);
  up(sp.chunk_nobs, &ds->d_chunk_nobs);
  up(sp.chunk_obs_off, &ds->d_chunk_obs_off);
  up(sp.chunk_hdr, &c.chunk_hdr);  // (empty: the plan does not fit the record, chunk_hdr stays null)
  c.n_fac = cp.n_fac;
  c.n_chunks = cp.n_chunks;
  c.n_chunks_exact = cp.n_chunks_exact;
  c.n_generic = static_cast<int64_t>(cp.generic_subjects.size());
  c.G = cp.G;
  ds->cobs_size = sp.cobs_size;
}

}  // namespace

int32_t get_stream(pmx_population* pop, const pmx::CompileKey& key, const pmx::ClassTunables& ct, DeviceStream** out) {
  std::lock_guard<std::mutex> lock(pop->mu);
  for (auto& s : pop->streams)
    if (s->key == key) {
      *out = s.get();
      return PMX_OK;
    }
  const pmx::HostPopulation& hp = pop->hp;
  pmx::StreamPlan sp;
  std::string err;
  const int32_t rc = pmx::plan_stream(hp, key, ct, &sp, &err);
  if (rc != PMX_OK) return fail(rc, err);
  const pmx::OpStream& os = sp.os;
  auto ds = std::make_unique<DeviceStream>();
  ds->key = key;
  ds->f = facts_of(sp, key);
  Uploader up{&ds->allocs};
  pmx::DevOps& d = ds->dev;
  up(os.subj_op_off, &d.subj_op_off);
  up(hp.subj_obs_off, &d.subj_obs_off);
  up(os.subj_order, &d.subj_order);
  up(os.op_meta, &d.op_meta);
  up(os.op_a, &d.op_a);
  up(os.op_b, &d.op_b);
  up(os.op_n, &d.op_n);
  up(os.op_rate, &d.op_rate);
  up(sp.op_rec, &d.op_rec);
  up(os.op_fac, &d.op_fac);
  up(sp.op_kfac, &d.op_kfac);
  up(os.op_t0, &d.op_t0);
  up(os.op_t1, &d.op_t1);
  up(os.lagb_off, &d.lagb_off);
  up(os.lagb_time, &d.lagb_time);
  up(os.lagb_amount, &d.lagb_amount);
  if (key.lag_merge) up(os.lagb_input, &d.lagb_input);
  d.n_rate = key.n_rate;
  d.n_cov = 0;
  if ((key.eq_kind == PMX_EQ_ODE || key.user_cov) && hp.n_cov > 0) {  // covariate segments for bodies that read them on the device
    d.n_cov = hp.n_cov;
    up(hp.cov_seg_off, &d.cov_seg_off);
    up(hp.seg_from, &d.seg_from);
    up(hp.seg_to, &d.seg_to);
    up(hp.seg_slope, &d.seg_slope);
    up(hp.seg_icpt, &d.seg_icpt);
    up(hp.cov_first_t, &d.cov_first_t);
    up(hp.cov_first_v, &d.cov_first_v);
  }
  up(sp.subj_step_off, &ds->steps.subj_step_off);
  up(sp.step_rec, &ds->steps.step_rec);
  if (sp.cp.n_chunks > 0) upload_class_plan(sp, ds.get(), up);
  if (up.rc != PMX_OK) return up.rc;
  *out = ds.get();
  pop->streams.push_back(std::move(ds));
  return PMX_OK;
}

int32_t acquire_ll_slot(const pmx_model* model, pmx_population* pop, DeviceStream* ds, const pmx_error_model* em,
                        void* stream, DeviceStream::LLCache** out, bool batch) {
  const int nout = model->d.nout;
  const auto& hp = pop->hp;
  std::lock_guard<std::mutex> lock(pop->mu);
  if (!pop->ll_ready) {  // observation-side inputs, once per population
    int32_t rc;
    std::vector<int32_t> oq(hp.obs_outeq.begin(), hp.obs_outeq.end());
    if ((rc = upload(hp.obs_value, &pop->d_obs_y, &pop->ll_allocs)) != PMX_OK) return rc;
    if ((rc = upload(oq, &pop->d_obs_outeq, &pop->ll_allocs)) != PMX_OK) return rc;
    if ((rc = upload(hp.obs_errorpoly, &pop->d_obs_poly, &pop->ll_allocs)) != PMX_OK) return rc;
    if ((rc = upload(hp.obs_censor, &pop->d_obs_cens, &pop->ll_allocs)) != PMX_OK) return rc;
    for (int64_t r = 0; r < hp.n_obs; ++r) {
      if (std::isnan(hp.obs_value[static_cast<size_t>(r)])) continue;
      const int q = hp.obs_outeq[static_cast<size_t>(r)];
      if (q >= 0 && q < 32) pop->valued_outeq_mask |= (1u << q);
      if (!hp.obs_censor.empty() && hp.obs_censor[static_cast<size_t>(r)] != PMX_CENSOR_NONE) pop->any_censored = true;
    }
    pop->ll_ready = true;
  }
  for (int q = 0; q < 32; ++q) {
    if (!((pop->valued_outeq_mask >> q) & 1u)) continue;
    if (q >= nout) return fail(PMX_ERR_OUTEQ_OUT_OF_RANGE, "observation outeq >= nout");
    // log_likelihood_matrix: MissingErrorModel fails the call (error_model.rs:1045-1080 through matrix.rs:83,104).
    // log_likelihood_batch: ResidualErrorModels::total_log_likelihood gives such a SUBJECT -inf and the call succeeds
    // (residual_error.rs:413-425): the table fill poisons the rows of that output (pmx_ll_prepare_obs), the subject's sum
    // comes out NaN with PMX_PAIR_NONFINITE, the batch entry points map that to -inf.
    if (!batch && (em[q].kind < PMX_EM_ADDITIVE || em[q].kind > PMX_EM_RES_EXPONENTIAL))
      return fail(PMX_ERR_ERROR_MODEL, "MissingErrorModel: output " + std::to_string(q) + " has observations but no error model");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  DeviceStream::LLCache* slot = nullptr;
  for (auto& c : ds->ll_cache)
    if (static_cast<int>(c.em.size()) == nout && std::memcmp(c.em.data(), em, sizeof(pmx_error_model) * nout) == 0) {
      slot = &c;
      break;
    }
  const bool hit = slot != nullptr;
  if (!hit) {
    constexpr size_t kSlots = 4;
    if (ds->ll_cache.size() >= kSlots)  // least recently used slot nobody is about to launch on
      for (auto& c : ds->ll_cache)
        if (c.host_users == 0 && (slot == nullptr || c.stamp < slot->stamp)) slot = &c;
    if (slot == nullptr) {
      ds->ll_cache.emplace_back();
      slot = &ds->ll_cache.back();
      void* p = nullptr;
      PMX_HIP(hipMalloc(&p, static_cast<size_t>(hp.n_obs > 0 ? hp.n_obs : 1) * 4 * sizeof(double)));
      ds->allocs.push_back(p);
      slot->d_obs = static_cast<double*>(p);
      if (ds->cobs_size > 0) {
        // (+ 2 G doubles of slack: the kernel requests a step's observation block before it knows the step has one)
        PMX_HIP(hipMalloc(&p, static_cast<size_t>(ds->cobs_size + 2 * ds->cls.G) * sizeof(double)));
        ds->allocs.push_back(p);
        slot->d_cobs = static_cast<double*>(p);
      }
      PMX_HIP(hipMalloc(&p, sizeof(int32_t)));
      ds->allocs.push_back(p);
      slot->d_err = static_cast<int32_t*>(p);
      PMX_HIP(hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming));
      PMX_HIP(hipEventRecord(slot->ev, st));
    }
  }
  PMX_HIP(hipStreamWaitEvent(st, slot->ev, 0));  // after the slot's last fill / read, whatever stream that was on
  if (!hit) {
    pmx::LLPrepareArgs a{};
    a.obs_y = pop->d_obs_y;
    a.obs_outeq = pop->d_obs_outeq;
    a.obs_poly = pop->d_obs_poly;
    a.obs_cens = pop->d_obs_cens;
    for (int q = 0; q < PMX_MAX_OUT; ++q) a.em[q] = q < nout ? em[q] : pmx_error_model{};
    a.n_obs = hp.n_obs;
    a.obs4 = slot->d_obs;
    a.err = slot->d_err;
    a.chunk_row = ds->cls.chunk_row;
    a.chunk_n = ds->cls.chunk_n;
    a.chunk_nobs = ds->d_chunk_nobs;
    a.chunk_obs_off = ds->d_chunk_obs_off;
    a.chunk_cls = ds->cls.chunk_cls;
    a.cls_prog_off = ds->cls.cls_prog_off;
    a.prog_meta = ds->cls.prog_meta;
    a.n_chunks = ds->cobs_size > 0 ? ds->cls.n_chunks : 0;
    a.G = ds->cls.G;
    a.cobs = slot->d_cobs;
    a.stream = stream;
    // Filling: until the event below is recorded behind the fill, the slot must not be hit by another host thread (its
    // stream would only wait for the slot's PREVIOUS use and read a half-written table).  pop->mu is held throughout; a
    // failed fill leaves the slot keyless.
    slot->em.clear();
    hipError_t fe = hipMemsetAsync(slot->d_err, 0, sizeof(int32_t), st);
    if (fe == hipSuccess) fe = pmx::launch_ll_prepare(a);
    if (fe == hipSuccess) fe = hipEventRecord(slot->ev, st);
    if (fe != hipSuccess) return fail(PMX_ERR_HIP, std::string("log-likelihood table fill: ") + hipGetErrorString(fe));
    slot->em.assign(em, em + nout);
  }
  slot->stamp = ++ds->ll_stamp;
  slot->host_users++;
  *out = slot;
  return PMX_OK;
}

int32_t resident_obs_off(pmx_population* pop) {
  std::lock_guard<std::mutex> lock(pop->mu);
  if (pop->d_subj_obs_off != nullptr) return PMX_OK;
  const auto& off = pop->hp.subj_obs_off;
  int64_t most = 0;
  for (size_t s = 0; s + 1 < off.size(); ++s) most = off[s + 1] - off[s] > most ? off[s + 1] - off[s] : most;
  const int32_t rc = upload(off, &pop->d_subj_obs_off, &pop->ll_allocs);
  if (rc == PMX_OK) pop->max_subject_rows = most;
  return rc;
}

namespace {

// under pop->mu.  Prediction rows are the observations in event order, so a walk over a subject's occasions counts them;
// within an occasion a stable sort by outeq keeps each profile's rows in prediction order.
void build_profiles(pmx_population* pop) {
  auto& pr = pop->profiles;
  if (pr.built) return;
  const auto& hp = pop->hp;
  pr.off.assign(1, 0);
  pr.row.reserve(static_cast<size_t>(hp.n_obs));
  pr.time.reserve(static_cast<size_t>(hp.n_obs));
  std::vector<std::pair<int32_t, int64_t>> obs;  // (outeq, row) of one occasion
  for (int64_t s = 0; s < hp.n_subjects; ++s) {
    int64_t r = hp.subj_obs_off[static_cast<size_t>(s)];
    for (int64_t o = hp.subj_occ_off[static_cast<size_t>(s)]; o < hp.subj_occ_off[static_cast<size_t>(s) + 1]; ++o) {
      obs.clear();
      for (int64_t e = hp.occ_ev_off[static_cast<size_t>(o)]; e < hp.occ_ev_off[static_cast<size_t>(o) + 1]; ++e)
        if (hp.ev_kind[static_cast<size_t>(e)] == PMX_EV_OBSERVATION) obs.emplace_back(hp.ev_io[static_cast<size_t>(e)], r++);
      std::stable_sort(obs.begin(), obs.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      for (size_t k = 0; k < obs.size(); ++k) {
        if (k == 0 || obs[k].first != obs[k - 1].first) {
          if (k > 0) pr.off.push_back(static_cast<int64_t>(pr.row.size()));
          pr.subject.push_back(s);
          pr.occasion.push_back(o - hp.subj_occ_off[static_cast<size_t>(s)]);
          pr.outeq.push_back(obs[k].first);
        }
        pr.row.push_back(obs[k].second);
        pr.time.push_back(hp.obs_time[static_cast<size_t>(obs[k].second)]);
      }
      if (!obs.empty()) pr.off.push_back(static_cast<int64_t>(pr.row.size()));
    }
  }
  pr.built = true;
}

}  // namespace

void host_profiles(pmx_population* pop) {
  std::lock_guard<std::mutex> lock(pop->mu);
  build_profiles(pop);
}

int32_t resident_profiles(pmx_population* pop) {
  std::lock_guard<std::mutex> lock(pop->mu);
  build_profiles(pop);
  auto& pr = pop->profiles;
  if (pr.resident) return PMX_OK;
  Uploader up{&pop->ll_allocs};
  up(pr.off, &pr.d_off);
  up(pr.row, &pr.d_row);
  up(pr.time, &pr.d_time);
  up(pr.subject, &pr.d_subject);
  if (up.rc == PMX_OK) pr.resident = true;
  return up.rc;
}

void release_ll_slot(pmx_population* pop, DeviceStream::LLCache* slot, void* stream) {
  std::lock_guard<std::mutex> lock(pop->mu);
  (void)hipEventRecord(slot->ev, static_cast<hipStream_t>(stream));
  slot->host_users--;
}

// pmx_host.cpp — the HOST-pointer entry points of include/pmx.h: pmx_predict, pmx_predict_batch, pmx_loglik,
// pmx_loglik_batch, pmx_mixture_loglik, pmx_dfunction, pmx_summarize_predictions, pmx_exposure_attainment.  Each uploads theta, runs the same enqueue as its *_device twin on a private stream and copies the
// result out.
#include <cstring>
#include <limits>

#include "pmx_internal.hpp"

// What they keep between calls, per population: device buffers for theta / output / status (grown, never shrunk), a private stream pair and
// two pinned bounce buffers.  An NPAG loop calls these entry points thousands of times; allocating, page-locking and
// freeing per call cost ~700x the kernel (profiles/r01/pcie_inclusive.txt).  Calls on one population take turns.
struct HostWorkspace {
  std::mutex mu;
  hipStream_t compute = nullptr, copy = nullptr;
  void* d_theta = nullptr;
  void* d_out = nullptr;
  void* d_status = nullptr;
  void* d_red = nullptr;      // the reductions' small vectors: weights or lpyl in, lpyl or D out, the D-function's slabs
  int32_t* d_flag = nullptr;  // "any pair failed" (pmx_status_any)
  size_t theta_cap = 0, out_cap = 0, status_cap = 0, red_cap = 0;
  static constexpr size_t kBounce = 32u << 20;
  void* bounce[2] = {nullptr, nullptr};
  hipEvent_t bev[2] = {nullptr, nullptr};
  int32_t* h_flag = nullptr;  // pinned
  ~HostWorkspace() {
    if (d_theta) (void)hipFree(d_theta);
    if (d_out) (void)hipFree(d_out);
    if (d_status) (void)hipFree(d_status);
    if (d_red) (void)hipFree(d_red);
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

extern "C" void pmx_population_destroy(pmx_population* pop) {
  if (!pop) return;
  {
    DeviceGuard g;
    (void)g.enter(pop->device);
    pop->streams.clear();
    pop->ws.reset();
  }
  delete pop;
}

namespace {

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
  HostWorkspace* ws = nullptr;
  ~WsDrain() {
    if (!ws) return;
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

// One host-pointer call: the caller's device, this population's workspace for the length of the call (calls on one
// population take turns), theta on the device and a zeroed status array - then the kernels, then finish().  The members
// go in reverse order: drain, end of turn, the caller's device back.
struct HostCall {
  DeviceGuard guard;
  std::unique_lock<std::mutex> turn;
  WsDrain drain;
  HostWorkspace* ws = nullptr;
  int64_t Pd = 1;  // columns of the dense device matrix; the caller's padding columns are never touched
  size_t n_status = 0, rows = 0;
  double* d_out() const { return static_cast<double*>(ws->d_out); }

  // out_rows: rows of the result (observations, or subjects); matrix shape [out_rows][P], batch shape [out_rows]
  int32_t begin(const pmx_model* model, pmx_population* pop, const double* theta, int64_t P, int batch, int64_t out_rows) {
    PMX_HIP(guard.enter(pop->device));
    int32_t rc = ws_get(pop, &ws);
    if (rc != PMX_OK) return rc;
    turn = std::unique_lock<std::mutex>(ws->mu);
    drain.ws = ws;
    const int64_t S = pop->hp.n_subjects;
    Pd = batch ? 1 : P;
    rows = static_cast<size_t>(out_rows);
    n_status = static_cast<size_t>(S * Pd);
    const size_t theta_bytes = static_cast<size_t>(batch ? S : P) * model->d.nparams * sizeof(double);
    if ((rc = ws_reserve(&ws->d_theta, &ws->theta_cap, theta_bytes)) != PMX_OK) return rc;
    if ((rc = ws_reserve(&ws->d_out, &ws->out_cap, rows * Pd * sizeof(double))) != PMX_OK) return rc;
    if ((rc = ws_reserve(&ws->d_status, &ws->status_cap, n_status)) != PMX_OK) return rc;
    PMX_HIP(hipMemcpyAsync(ws->d_theta, theta, theta_bytes, hipMemcpyHostToDevice, ws->compute));
    if (n_status > 0) PMX_HIP(hipMemsetAsync(ws->d_status, 0, n_status, ws->compute));
    return PMX_OK;
  }
  int32_t run(const pmx_model* model, pmx_population* pop, int64_t P, int batch, const LLRequest* req = nullptr) {
    return enqueue(model, pop, static_cast<const double*>(ws->d_theta), P, batch, d_out(), Pd, static_cast<uint8_t*>(ws->d_status),
                   ws->compute, req);
  }
  // the status flag (and array, if asked for), then the result into the caller's rows `ld` doubles apart
  int32_t finish(uint8_t* status, double* out, int64_t ld, bool* any_failed) {
    const int32_t rc = ws_finish_status(ws, status, n_status, any_failed);
    if (rc != PMX_OK) return rc;
    return ws_copy_out(ws, out, static_cast<size_t>(ld) * sizeof(double), ws->d_out, static_cast<size_t>(Pd) * sizeof(double), rows);
  }
};

constexpr const char* kPairFailed = "at least one (subject, support point) pair failed; see the status array";

int32_t predict_host(const pmx_model* model, const pmx_population* cpop, const double* theta, int64_t P, int batch,
                     double* pred, int64_t ld, uint8_t* status) {
  pmx::clear_error();
  if (!model || !cpop || !theta || !pred) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!batch && (P <= 0 || ld < P)) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_pred >= n_support");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  HostCall call;
  int32_t rc = call.begin(model, pop, theta, P, batch, pop->hp.n_obs);
  if (rc == PMX_OK) rc = call.run(model, pop, P, batch);
  bool any_failed = false;
  if (rc == PMX_OK) rc = call.finish(status, pred, ld, &any_failed);
  if (rc != PMX_OK) return rc;
  return any_failed ? fail(PMX_ERR_PAIR_FAILED, kPairFailed) : PMX_OK;
}

// The log-likelihood part every host form shares: begin, the kernels, and the invalid-sigma counter read back.  On
// PMX_OK call.d_out() holds ll[s][p] (matrix shape, dense) or ll[s] (batch shape: subject s with theta row s,
// likelihood/mod.rs:119-177) on the device, ordered on call.ws->compute.
int32_t loglik_into(HostCall& call, const pmx_model* model, pmx_population* pop, const pmx_error_model* em, int64_t P,
                    int batch, double* d_ll);
int32_t loglik_on_device(HostCall& call, const pmx_model* model, pmx_population* pop, const pmx_error_model* em,
                         const double* theta, int64_t P, int batch) {
  const int32_t rc = call.begin(model, pop, theta, P, batch, pop->hp.n_subjects);
  return rc != PMX_OK ? rc : loglik_into(call, model, pop, em, P, batch, call.d_out());
}

// ... after begin(): the kernels write the dense d_ll (rows call.Pd apart) from the theta and into the status begin() set up
int32_t loglik_into(HostCall& call, const pmx_model* model, pmx_population* pop, const pmx_error_model* em, int64_t P,
                    int batch, double* d_ll) {
  int32_t rc;
  HostWorkspace* ws = call.ws;
  const int32_t* d_sigma_err = nullptr;
  LLRequest req{em, d_ll, call.Pd, &d_sigma_err};
  if ((rc = enqueue(model, pop, static_cast<const double*>(ws->d_theta), P, batch, d_ll, call.Pd,
                    static_cast<uint8_t*>(ws->d_status), ws->compute, &req)) != PMX_OK)
    return rc;
  if (d_sigma_err) {  // ErrorModelError::NegativeSigma / NonFiniteSigma (error_model.rs:1073-1077), found on the device
    PMX_HIP(hipMemcpyAsync(ws->h_flag, d_sigma_err, sizeof(int32_t), hipMemcpyDeviceToHost, ws->compute));
    PMX_HIP(hipStreamSynchronize(ws->compute));
    const int32_t n_bad = *ws->h_flag;
    if (n_bad > 0)
      return fail(PMX_ERR_ERROR_MODEL, "NegativeSigma / NonFiniteSigma for " + std::to_string(n_bad) + " observation(s)");
  }
  return PMX_OK;
}

int32_t loglik_host(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em, const double* theta,
                    int64_t P, int batch, double* ll, int64_t ld_ll, uint8_t* status) {
  pmx::clear_error();
  if (!model || !cpop || !em || !theta || !ll) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!batch && (P <= 0 || ld_ll < P)) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0 and ld_ll >= n_support");
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  HostCall call;
  int32_t rc = loglik_on_device(call, model, pop, em, theta, P, batch);
  if (rc != PMX_OK) return rc;
  HostWorkspace* ws = call.ws;
  bool any_failed = false;
  if ((rc = call.finish(status, ll, ld_ll, &any_failed)) != PMX_OK) return rc;
  if (!any_failed) return PMX_OK;
  if (!batch) return fail(PMX_ERR_PAIR_FAILED, kPairFailed);
  // log_likelihood_batch maps a failed subject to -inf instead of failing the call (likelihood/mod.rs:137-140):
  // the status array names them, the caller's row is overwritten here
  std::vector<uint8_t> hst(call.n_status);
  PMX_HIP(hipMemcpy(hst.data(), ws->d_status, call.n_status, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < call.n_status; ++i)
    if (hst[i] != PMX_PAIR_OK) ll[i] = -std::numeric_limits<double>::infinity();
  return PMX_OK;
}

// A reduction of the matrix a host form left on the device (pmx_mixture.hip): `in` [n_in] goes up, the kernels run on
// the workspace's [n_in | n_out | n_scratch] doubles, `out` [n_out] comes back - with the status flag (and array) of
// pmx_loglik; the matrix never crosses the link.
template <class Launch>
int32_t reduce_host(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em, const double* theta,
                    int64_t P, const double* in, int64_t n_in, double* out, int64_t n_out, int64_t n_scratch,
                    uint8_t* status, Launch&& launch) {
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  HostCall call;
  int32_t rc = loglik_on_device(call, model, pop, em, theta, P, 0);
  if (rc != PMX_OK) return rc;
  HostWorkspace* ws = call.ws;
  if ((rc = ws_reserve(&ws->d_red, &ws->red_cap, static_cast<size_t>(n_in + n_out + n_scratch) * sizeof(double))) != PMX_OK)
    return rc;
  double* d_in = static_cast<double*>(ws->d_red);
  double* d_res = d_in + n_in;
  PMX_HIP(hipMemcpyAsync(d_in, in, static_cast<size_t>(n_in) * sizeof(double), hipMemcpyHostToDevice, ws->compute));
  PMX_HIP(launch(call.d_out(), d_in, d_res, d_res + n_out, ws->compute));
  bool any_failed = false;
  if ((rc = ws_finish_status(ws, status, call.n_status, &any_failed)) != PMX_OK) return rc;
  const size_t out_bytes = static_cast<size_t>(n_out) * sizeof(double);
  if ((rc = ws_copy_out(ws, out, out_bytes, d_res, out_bytes, 1)) != PMX_OK) return rc;
  return any_failed ? fail(PMX_ERR_PAIR_FAILED, kPairFailed) : PMX_OK;
}

// weights arrive on the host: a negative or NaN entry, or no positive one, is refused before any work
int32_t check_weights(const double* w, int64_t n) {
  bool any_positive = false;
  for (int64_t p = 0; p < n; ++p) {
    if (!(w[p] >= 0.0)) return fail(PMX_ERR_INVALID_ARGUMENT, "w[" + std::to_string(p) + "] is negative or NaN");
    any_positive = any_positive || w[p] > 0.0;
  }
  return any_positive ? PMX_OK : fail(PMX_ERR_INVALID_ARGUMENT, "w holds no positive entry");
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
int32_t pmx_loglik(const pmx_model* model, const pmx_population* pop, const pmx_error_model* em, const double* theta,
                   int64_t n_support, double* ll, int64_t ld_ll, uint8_t* status) {
  return loglik_host(model, pop, em, theta, n_support, 0, ll, ld_ll, status);
}
int32_t pmx_loglik_batch(const pmx_model* model, const pmx_population* pop, const pmx_error_model* em, const double* theta,
                         double* ll, uint8_t* status) {
  return loglik_host(model, pop, em, theta, 1, 1, ll, 1, status);
}

int32_t pmx_mixture_loglik(const pmx_model* model, const pmx_population* pop, const pmx_error_model* em, const double* theta,
                           int64_t n_support, const double* w, double* lpyl, uint8_t* status) {
  pmx::clear_error();
  if (!model || !pop || !em || !theta || !w || !lpyl) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_support <= 0) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0");
  const int32_t rc = check_weights(w, n_support);
  if (rc != PMX_OK) return rc;
  const int64_t S = pop->hp.n_subjects;
  return reduce_host(model, pop, em, theta, n_support, w, n_support, lpyl, S, 0, status,
                     [&](const double* d_ll, const double* d_w, double* d_lpyl, double*, hipStream_t st) {
                       return pmx::launch_mixture_rows(d_ll, S, n_support, n_support, d_w, d_lpyl, st);
                     });
}

int32_t pmx_dfunction(const pmx_model* model, const pmx_population* pop, const pmx_error_model* em, const double* theta,
                      int64_t n_cand, const double* lpyl, double* D, uint8_t* status) {
  pmx::clear_error();
  if (!model || !pop || !em || !theta || !lpyl || !D) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (n_cand <= 0) return fail(PMX_ERR_INVALID_ARGUMENT, "n_cand must be > 0");
  const int64_t S = pop->hp.n_subjects;
  const int64_t n_scratch = S > 0 ? pmx::dfunction_tiles(S, n_cand) * n_cand : 0;
  return reduce_host(model, pop, em, theta, n_cand, lpyl, S, D, n_cand, n_scratch, status,
                     [&](const double* d_ll, const double* d_lpyl, double* d_D, double* d_scratch, hipStream_t st) {
                       return pmx::launch_dfunction(d_ll, S, n_cand, n_cand, d_lpyl, d_scratch, d_D, st);
                     });
}

// predict, then - posterior mode - loglik and the mixture rows, then the summaries (pmx_posterior.hip), all on the
// private stream: pred stays in the workspace's output matrix, ll and the small vectors in its reduction buffer
// [w | lpyl | mean | median | ll], and n_observations doubles come back per requested output.
int32_t pmx_summarize_predictions(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                                  const double* theta, int64_t n_support, const double* w, double* mean, double* median,
                                  uint8_t* status) {
  pmx::clear_error();
  if (!model || !cpop || !theta || !w) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!mean && !median) return fail(PMX_ERR_INVALID_ARGUMENT, "mean and median are both null: nothing to compute");
  if (n_support <= 0) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0");
  int32_t rc = check_weights(w, n_support);
  if (rc != PMX_OK) return rc;
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  const int64_t S = pop->hp.n_subjects, n_obs = pop->hp.n_obs, P = n_support;
  HostCall call;
  if ((rc = call.begin(model, pop, theta, P, 0, n_obs)) != PMX_OK) return rc;
  if ((rc = call.run(model, pop, P, 0)) != PMX_OK) return rc;
  HostWorkspace* ws = call.ws;
  const size_t n_red = static_cast<size_t>(P + S + 2 * n_obs + (em ? S * P : 0));
  if ((rc = ws_reserve(&ws->d_red, &ws->red_cap, n_red * sizeof(double))) != PMX_OK) return rc;
  double* d_w = static_cast<double*>(ws->d_red);
  double* d_lpyl = d_w + P;
  double* d_mean = d_lpyl + S;
  double* d_median = d_mean + n_obs;
  double* d_ll = d_median + n_obs;
  PMX_HIP(hipMemcpyAsync(d_w, w, static_cast<size_t>(P) * sizeof(double), hipMemcpyHostToDevice, ws->compute));
  if (em) {
    if ((rc = loglik_into(call, model, pop, em, P, 0, d_ll)) != PMX_OK) return rc;
    PMX_HIP(pmx::launch_mixture_rows(d_ll, S, P, P, d_w, d_lpyl, ws->compute));
    if ((rc = resident_obs_off(pop)) != PMX_OK) return rc;
  }
  const pmx::SummaryArgs a{call.d_out(), n_obs, P, P, d_w, em ? d_ll : nullptr, P, em ? d_lpyl : nullptr, pop->d_subj_obs_off,
                           S, pop->max_subject_rows, mean ? d_mean : nullptr, median ? d_median : nullptr};
  PMX_HIP(pmx::launch_summary_rows(a, ws->compute));
  bool any_failed = false;
  if ((rc = ws_finish_status(ws, status, call.n_status, &any_failed)) != PMX_OK) return rc;
  const size_t out_bytes = static_cast<size_t>(n_obs) * sizeof(double);
  if (mean && (rc = ws_copy_out(ws, mean, out_bytes, d_mean, out_bytes, 1)) != PMX_OK) return rc;
  if (median && (rc = ws_copy_out(ws, median, out_bytes, d_median, out_bytes, 1)) != PMX_OK) return rc;
  return any_failed ? fail(PMX_ERR_PAIR_FAILED, kPairFailed) : PMX_OK;
}

// predict, then - posterior mode - loglik and the mixture rows, then the one exposure metric and its attainment
// (pmx_exposure.hip), all on the private stream: pred stays in the workspace's output matrix, the metric plane and the
// small vectors in its reduction buffer [w | lpyl | target | pta | mean | plane | ll], and n_profiles doubles come back
// per requested output.
int32_t pmx_exposure_attainment(const pmx_model* model, const pmx_population* cpop, const pmx_error_model* em,
                                const double* theta, int64_t n_support, const double* w, int32_t method,
                                const double* window, uint32_t metric, const double* target, double* pta, double* mean,
                                uint8_t* status) {
  pmx::clear_error();
  if (!model || !cpop || !theta || !w) return fail(PMX_ERR_INVALID_ARGUMENT, "null argument");
  if (!pta && !mean) return fail(PMX_ERR_INVALID_ARGUMENT, "pta and mean are both null: nothing to compute");
  if ((pta == nullptr) != (target == nullptr)) return fail(PMX_ERR_INVALID_ARGUMENT, "pta and target go together");
  if (n_support <= 0) return fail(PMX_ERR_INVALID_ARGUMENT, "n_support must be > 0");
  if (const char* why = exposure_refusal(method, window, metric)) return fail(PMX_ERR_INVALID_ARGUMENT, why);
  if ((metric & (metric - 1)) != 0) return fail(PMX_ERR_INVALID_ARGUMENT, "metric must be exactly one PMX_EXPO_* bit");
  int32_t rc = check_weights(w, n_support);
  if (rc != PMX_OK) return rc;
  pmx_population* pop = const_cast<pmx_population*>(cpop);
  const int64_t S = pop->hp.n_subjects, n_obs = pop->hp.n_obs, P = n_support;
  HostCall call;
  if ((rc = call.begin(model, pop, theta, P, 0, n_obs)) != PMX_OK) return rc;
  if ((rc = call.run(model, pop, P, 0)) != PMX_OK) return rc;
  if ((rc = resident_profiles(pop)) != PMX_OK) return rc;
  const auto& pr = pop->profiles;
  const int64_t n = pr.n();
  HostWorkspace* ws = call.ws;
  const size_t n_red = static_cast<size_t>(P + S + 3 * n + n * P + (em ? S * P : 0));
  if ((rc = ws_reserve(&ws->d_red, &ws->red_cap, n_red * sizeof(double))) != PMX_OK) return rc;
  double* d_w = static_cast<double*>(ws->d_red);
  double* d_lpyl = d_w + P;
  double* d_target = d_lpyl + S;
  double* d_pta = d_target + n;
  double* d_mean = d_pta + n;
  double* d_plane = d_mean + n;
  double* d_ll = d_plane + n * P;
  const size_t out_bytes = static_cast<size_t>(n) * sizeof(double);
  PMX_HIP(hipMemcpyAsync(d_w, w, static_cast<size_t>(P) * sizeof(double), hipMemcpyHostToDevice, ws->compute));
  if (target && n > 0) PMX_HIP(hipMemcpyAsync(d_target, target, out_bytes, hipMemcpyHostToDevice, ws->compute));
  if (em) {
    if ((rc = loglik_into(call, model, pop, em, P, 0, d_ll)) != PMX_OK) return rc;
    PMX_HIP(pmx::launch_mixture_rows(d_ll, S, P, P, d_w, d_lpyl, ws->compute));
  }
  const ExposureWindow win(window);
  const pmx::ExposureArgs ea{call.d_out(), P, P, pr.d_off, pr.d_row, pr.d_time, n, method, win.a, win.b, win.threshold, metric, d_plane, P};
  PMX_HIP(pmx::launch_exposure(ea, ws->compute));
  const pmx::AttainArgs aa{d_plane, n, P, P, pta ? d_target : nullptr, d_w, em ? d_ll : nullptr, P, em ? d_lpyl : nullptr,
                           pr.d_subject, pta ? d_pta : nullptr, mean ? d_mean : nullptr};
  PMX_HIP(pmx::launch_attainment(aa, ws->compute));
  bool any_failed = false;
  if ((rc = ws_finish_status(ws, status, call.n_status, &any_failed)) != PMX_OK) return rc;
  if (pta && (rc = ws_copy_out(ws, pta, out_bytes, d_pta, out_bytes, 1)) != PMX_OK) return rc;
  if (mean && (rc = ws_copy_out(ws, mean, out_bytes, d_mean, out_bytes, 1)) != PMX_OK) return rc;
  return any_failed ? fail(PMX_ERR_PAIR_FAILED, kPairFailed) : PMX_OK;
}

}  // extern "C"

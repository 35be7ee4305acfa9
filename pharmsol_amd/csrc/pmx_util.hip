// pmx_util.hip — small kernels beside the prediction grid: log-likelihood tables, status scan, streaming fill.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pmx_kernels.hpp"

namespace pmx {
// ------------------------------------------------------------------------------------
// log-likelihood tables (one thread per observation / per chunk slot)
// ------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void pmx_ll_prepare_obs(LLPrepareArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= a.n_obs) return;
  double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
  const double y = a.obs_y[r];
  if (y == y) {  // a valued observation (missing ones keep weight 0)
    const int q = a.obs_outeq[r];
    const pmx_error_model& e = a.em[q < PMX_MAX_OUT ? q : 0];
    if (e.kind < PMX_EM_ADDITIVE || e.kind > PMX_EM_RES_EXPONENTIAL) {
      // no error model for this output (only the batch entry points get here: log_likelihood_batch scores such a subject
      // -inf instead of failing, residual_error.rs:413-425): the row poisons its subject's sum
      const double nanq = __longlong_as_double(0x7ff8000000000000LL);
      a.obs4[r * 4 + 0] = nanq;
      a.obs4[r * 4 + 1] = nanq;
      a.obs4[r * 4 + 2] = 1.0;
      a.obs4[r * 4 + 3] = 0.0;
      return;
    }
    double c0 = e.c[0], c1 = e.c[1], c2 = e.c[2], c3 = e.c[3];
    if (a.obs_poly != nullptr) {  // the observation's own polynomial wins (error_model.rs:1051-1054)
      const double p0 = a.obs_poly[r * 4];
      if (p0 == p0) {
        c0 = p0;
        c1 = a.obs_poly[r * 4 + 1];
        c2 = a.obs_poly[r * 4 + 2];
        c3 = a.obs_poly[r * 4 + 3];
      }
    }
    if (e.kind >= PMX_EM_RES_CONSTANT) {  // residual models: the fold derives sigma from the prediction (ll_residual_term)
      a.obs4[r * 4 + 0] = y;
      a.obs4[r * 4 + 1] = e.scalar;
      a.obs4[r * 4 + 2] = -static_cast<double>(e.kind);
      a.obs4[r * 4 + 3] = e.c[0];
      return;
    }
    const double alpha = c0 + c1 * y + c2 * (y * y) + c3 * (y * y * y);
    const double sigma = (e.kind == PMX_EM_ADDITIVE) ? sqrt(alpha * alpha + e.scalar * e.scalar) : e.scalar * alpha;
    const int cz = a.obs_cens != nullptr ? a.obs_cens[r] : 0;
    const bool bad = !(sigma >= 0.0) || !isfinite(sigma) || (cz != 0 && !(sigma > 0.0));
    q0 = y;
    q1 = -0.5 * 1.8378770664093453 - log(sigma);
    q2 = 1.0 / (2.0 * sigma * sigma);
    q3 = (cz == 0) ? 0.0 : ((cz > 0 ? 1.0 : -1.0) / (sigma * 1.4142135623730951));
    if (bad) {  // NegativeSigma / NonFiniteSigma: the row (and so the subject's sum) becomes NaN
      q0 = q1 = __longlong_as_double(0x7ff8000000000000LL);  // (q0 too: the censored fold reads value and scale only)
      q2 = 1.0;
      atomicAdd(a.err, 1);
    }
  }
  a.obs4[r * 4 + 0] = q0;
  a.obs4[r * 4 + 1] = q1;
  a.obs4[r * 4 + 2] = q2;
  a.obs4[r * 4 + 3] = q3;
}

// A chunk's block of cobs: [G] csum, [G] flags, then [k][2][G] = {observed value, weight} of observation k of member j (0 for padding
// members and missing observations).  A plain row's term is  c - w (y - pred)^2 ; the constants c depend on nothing the
// kernel computes, so they are summed here, once per (error model, population), and the kernel adds csum[j] at the end.
// A censored row (BLOQ / ALOQ) or a residual-model row carries weight -1 as a marker: the kernel takes the row's full
// record {value, const, weight, censor scale} from obs4 (rare, out of the main path; its constant is not in csum).
__global__ __launch_bounds__(256) void pmx_ll_prepare_chunks(LLPrepareArgs a) {
  const int64_t ch = blockIdx.x;
  if (ch >= a.n_chunks) return;
  const int32_t nobs = a.chunk_nobs[ch], n_live = a.chunk_n[ch];
  const int64_t base = a.chunk_obs_off[ch];
  const int32_t total = nobs * 2 * a.G;
  for (int32_t i = threadIdx.x; i < total; i += 256) {
    const int32_t j = i % a.G, f = (i / a.G) % 2, k = i / (2 * a.G);
    double v = 0.0;
    if (j < n_live) {
      const double* rec = a.obs4 + (a.chunk_row[ch * a.G + j] + k) * 4;
      v = f == 0 ? rec[0] : rec[2];
      if (f == 1 && (rec[3] != 0.0 || rec[2] < 0.0) && v == v) v = -1.0;
    }
    a.cobs[base + 2 * a.G + i] = v;
  }
  if (threadIdx.x == 0) {
    // bit k: every live member's row of observation k is a plain one (weight neither 0 = missing nor the detour marker):
    // the kernel then folds the G members without a test per member
    uint64_t plain = 0;
    for (int32_t k = 0; k < nobs && k < 63; ++k) {
      bool all = true;
      for (int32_t j = 0; j < n_live; ++j) {
        const double* rec = a.obs4 + (a.chunk_row[ch * a.G + j] + k) * 4;
        const bool detour = (rec[3] != 0.0 || rec[2] < 0.0) && rec[2] == rec[2];
        all = all && !detour && __double_as_longlong(rec[2]) != 0;
      }
      if (all) plain |= (1ull << k);
    }
    a.cobs[base + a.G] = __longlong_as_double(static_cast<int64_t>(plain));
    // ... and the same mask indexed by program STEP (bit s < 63: step s carries an observation that is plain for every
    // live member), for the kernel that picks its straight-line steps by step number (pmx_analytical_classed_ll)
    uint64_t plain_step = 0;
    {
      const int32_t cl = a.chunk_cls[ch];
      int32_t k = 0;
      for (int64_t o = a.cls_prog_off[cl], s = 0; o < a.cls_prog_off[cl + 1]; ++o, ++s) {
        if ((a.prog_meta[o] >> kOpObsAfterShift) & 1u) {
          if (s < 63 && k < 63 && ((plain >> k) & 1ull)) plain_step |= 1ull << s;
          ++k;
        }
      }
    }
    a.cobs[base + a.G + 1] = __longlong_as_double(static_cast<int64_t>(plain_step));
    for (int32_t j = 2; j < a.G; ++j) a.cobs[base + a.G + j] = 0.0;
  }
  for (int32_t j = threadIdx.x; j < a.G; j += 256) {
    double csum = 0.0;
    if (j < n_live) {
      for (int32_t k = 0; k < nobs; ++k) {
        const double* rec = a.obs4 + (a.chunk_row[ch * a.G + j] + k) * 4;
        const bool detour = (rec[3] != 0.0 || rec[2] < 0.0) && rec[2] == rec[2];
        if (rec[2] != 0.0 && !detour) csum += rec[1];
      }
    }
    a.cobs[base + j] = csum;
  }
}
}  // namespace

hipError_t launch_ll_prepare(const LLPrepareArgs& a) {
  hipStream_t st = static_cast<hipStream_t>(a.stream);
  if (a.n_obs > 0) {
    hipLaunchKernelGGL(pmx_ll_prepare_obs, dim3(static_cast<uint32_t>((a.n_obs + 255) / 256)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.n_chunks > 0) {
    hipLaunchKernelGGL(pmx_ll_prepare_chunks, dim3(static_cast<uint32_t>(a.n_chunks)), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

namespace {
// any non-zero status byte -> *flag = 1 (16 bytes per lane per trip; n is tens of MB at most)
__global__ __launch_bounds__(256) void pmx_status_any(const uint8_t* __restrict__ st, int64_t n, int32_t* __restrict__ flag) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256 * 16;
  uint32_t acc = 0;
  for (int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 16; i < n; i += stride) {
    if (i + 16 <= n && (reinterpret_cast<uintptr_t>(st + i) & 15u) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(st + i);
      acc |= v.x | v.y | v.z | v.w;
    } else {
      for (int64_t j = i; j < n && j < i + 16; ++j) acc |= st[j];
    }
  }
  if (__any(acc != 0u ? 1 : 0) && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1);
}
}  // namespace

namespace {
// Streaming fills: what the device's write path takes when nothing else is asked of it (the measured ceiling bench.py
// prints beside the 8 TB/s datasheet peak: roofline.attainable).  Four shapes, the entry point reports the best:
//   0  grid-stride, 16 bytes per lane, streaming (nt) stores
//   1  the same with plain stores
//   2  the prediction kernels' own shape: one wave = 512 contiguous bytes per store (8 bytes per lane, nt), each
//      workgroup walking its own contiguous 64 KiB piece
//   3  shape 0 without the loop: one store per lane, as many workgroups as that takes
template <int SHAPE>
__global__ __launch_bounds__(256) void pmx_fill_linear(double* __restrict__ dst, int64_t n_pairs, double v) {
  typedef double dbl2 __attribute__((ext_vector_type(2)));
  if constexpr (SHAPE == 2) {
    constexpr int64_t kPiece = 8192;  // doubles per workgroup piece
    const int64_t n = n_pairs * 2;
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kPiece; base < n; base += static_cast<int64_t>(gridDim.x) * kPiece) {
#pragma unroll 4
      for (int64_t i = threadIdx.x; i < kPiece; i += 256)
        if (base + i < n) __builtin_nontemporal_store(v, dst + base + i);
    }
  } else {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    dbl2 vv;
    vv.x = v;
    vv.y = v;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n_pairs; i += stride) {
      if constexpr (SHAPE == 0)
        __builtin_nontemporal_store(vv, reinterpret_cast<dbl2*>(dst) + i);
      else
        reinterpret_cast<dbl2*>(dst)[i] = vv;
    }
  }
}

__global__ void pmx_fill_one(double* dst, double v) { *dst = v; }
}  // namespace

hipError_t launch_fill_one(double* d_dst, double v, void* stream) {
  hipLaunchKernelGGL(pmx_fill_one, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), d_dst, v);
  return hipGetLastError();
}

hipError_t launch_fill_linear(double* d_dst, int64_t n_doubles, double v, void* stream, int shape) {
  const int64_t n_pairs = n_doubles / 2;
  if (n_pairs <= 0) return hipSuccess;
  int64_t blocks = shape == 2 ? (n_doubles + 8191) / 8192 : (n_pairs + 255) / 256;
  if (shape == 3) {  // one 16-byte streaming store per lane, no loop: the fastest of the shapes tried (tools/experiments/fill_probe.hip:
    shape = 0;       // 6.7 TB/s where the grid-stride forms reach 5.6-6.2 and hipMemsetAsync 6.4)
    if (blocks > 0x7fffffff) blocks = 0x7fffffff;
  } else if (blocks > 256 * 64) {
    blocks = 256 * 64;
  }
  const dim3 g(static_cast<uint32_t>(blocks)), b(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (shape == 0) hipLaunchKernelGGL(pmx_fill_linear<0>, g, b, 0, st, d_dst, n_pairs, v);
  if (shape == 1) hipLaunchKernelGGL(pmx_fill_linear<1>, g, b, 0, st, d_dst, n_pairs, v);
  if (shape == 2) hipLaunchKernelGGL(pmx_fill_linear<2>, g, b, 0, st, d_dst, n_pairs, v);
  return hipGetLastError();
}

hipError_t launch_status_any(const uint8_t* d_status, int64_t n, int32_t* d_flag, void* stream) {
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pmx_status_any, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), d_status, n, d_flag);
  return hipGetLastError();
}

}  // namespace pmx

// pmx_dyn3.hip — the matrix-free three-compartment covariate walker (GRID lane mapping).
#include "pmx_lanes.hpp"

namespace pmx {

namespace {

// ------------------------------------------------------------------------------------
// Three-compartment structures with covariate-derived rate constants on a population WITHOUT infusions (oral / bolus
// dosing: C5).  Every segment rebuilds its propagator and applies it once, so no transition matrix is formed: the
// matrix-free step of pmx_structures.hpp (ThreeNewton) - eigenvalues, the divided differences of exp(-l dt) on them and
// three sparse matrix-vector products.  Same lane mapping, op stream, kept-propagator codes and status rules as
// pmx_analytical_grid<KID, dyn>; a kept segment holds 6-7 numbers per lane in LDS instead of 12-16.  The host picks it
// when the compiled stream holds no PROP with a rate (LaunchArgs::no_rates) and the model has no pm_ pad slot.
// ------------------------------------------------------------------------------------
#ifndef PMX_DYN3_WAVES
#define PMX_DYN3_WAVES 3
#endif
// EIGR: the stream marks segments whose rate constants equal those of the occasion's previous built segment (bit 27: a
// subject-constant covariate) - the eigenvalues are kept in registers and only the divided differences are rebuilt
// (C5 with one wt per subject 10.6 -> 9.5 ms).  Its own instantiation: carrying the six registers and the second copy of
// the rebuild through the time-varying case cost that one 5 % (10.57 -> 11.09 ms).
template <int KID, bool LL, bool EIGR>
__global__ __launch_bounds__(kBlock, PMX_DYN3_WAVES) void pmx_analytical_dyn3(DevModel m, DevOps ops, const double* __restrict__ theta,
                                                                             int64_t P, int64_t S, int32_t s_chunk, int32_t n_ptiles,
                                                                             double* __restrict__ pred, int64_t ld,
                                                                             uint8_t* __restrict__ status,
                                                                             const int32_t* __restrict__ subj_list, int32_t zero_status,
                                                                             int32_t prop_slots) {
  using LM = LaneModel<KID>;
  constexpr int NS = LM::NS;
  constexpr int ND0 = LM::S::ND0;
  const int64_t b = blockIdx.x;
  const int32_t ptile = static_cast<int32_t>(b % n_ptiles);
  const int64_t chunk = b / n_ptiles;
  const uint32_t tile = blockDim.x;
  const int64_t p = static_cast<int64_t>(ptile) * tile + threadIdx.x;
  const bool lane_ok = p < P;
  const int64_t pc = lane_ok ? p : (P - 1);
  const double* __restrict__ th = theta + pc * m.nparams;
  extern __shared__ double prop_cache[];  // [slot][ND0][lane]
  (void)prop_cache;

  LM L;
  lane_setup<KID, true>(m, th, L);
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);
  const auto c_subj_op_off = as_const(ops.subj_op_off);
  const auto c_subj_obs_off = as_const(ops.subj_obs_off);

  const int64_t s_begin = chunk * s_chunk;
  const int64_t s_end = (s_begin + s_chunk < S) ? (s_begin + s_chunk) : S;
  // An op = its 4-byte meta word + its 64-byte record {factor of kernel parameter 0..6, op_a} (DevOps::op_kfac), both
  // requested ONE OP AHEAD: a scalar fetch of a line nobody touched before costs about a microsecond, and with one in
  // front of every rebuild the walker waited on the scalar cache more than it computed.  Without a subject list the
  // stream is walked in order, so the look-ahead runs across subjects (a subject's last op requests the next one's first).
  const bool chained = subj_list == nullptr;
  const int64_t o_blk_end = chained ? c_subj_op_off[s_end] : 0;  // (the look-ahead never leaves the ops of this block's subjects:
                                                                 // trailing subjects without ops would otherwise send it one past the stream)
  uint32_t meta_n = 0u;
  u32x16 rec_n = {};
  // ... and so does the subject's header {first op, end op, first row}: the next subject's end op and first row are
  // requested while this one is walked (its first op is this one's end op)
  int64_t o0_n = 0, o1_n = 0, row_n = 0;
  bool primed = false;
  if (chained && s_begin < s_end) {
    o0_n = sload_here<int64_t>(ops.subj_op_off + s_begin);
    o1_n = sload_here<int64_t>(ops.subj_op_off + s_begin + 1);
    row_n = sload_here<int64_t>(ops.subj_obs_off + s_begin);
  }
  for (int64_t si = s_begin; si < s_end; ++si) {
    const int64_t s = subj_list ? static_cast<int64_t>(as_const(subj_list)[si]) : si;
    int64_t o0, o1, row;
    if (chained) {
      o0 = o0_n;
      o1 = o1_n;
      row = row_n;
      asm volatile("" : "+s"(o0), "+s"(o1), "+s"(row));
      const int64_t sn = (si + 1 < s_end) ? s + 1 : s;  // (the last subject of the block requests itself again)
      o0_n = o1;
      o1_n = sload_here<int64_t>(ops.subj_op_off + sn + 1);
      row_n = sload_here<int64_t>(ops.subj_obs_off + sn);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      o0 = c_subj_op_off[s];
      o1 = c_subj_op_off[s + 1];
      row = c_subj_obs_off[s];
    }
    if ((!chained || !primed) && o0 < o1) {  // (chained: once, at the block's first subject that has any op)
      meta_n = sload_here<uint32_t>(ops.op_meta + o0);
      rec_n = sload_here<u32x16>(ops.op_kfac + o0 * 8);
      primed = true;
    }
    double x[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = 0.0;
    double ll_acc = 0.0;
    double lprev[3] = {0.0, 0.0, 0.0};  // eigenvalues of the occasion's last built segment (bit 27 of a PROP reuses them)
    bool okprev = true;
    uint8_t st = PMX_PAIR_OK;
    uint8_t st_sticky = PMX_PAIR_OK;  // first failure of an EARLIER occasion (the reference errors out for the whole subject)
    if (zero_status == 1 && status != nullptr) {  // (status protocol: pmx_analytical_grid)
      const uint32_t zl = threadIdx.x & 63u;
      const int64_t zp = static_cast<int64_t>(ptile) * tile + (threadIdx.x & ~63u) + 8 * zl;
      if (zl < 8u && zp < P) *reinterpret_cast<uint64_t*>(status + s * P + zp) = 0ull;
    }
    for (int64_t o = o0; o < o1; ++o) {
      uint32_t meta = meta_n;
      u32x16 rec = rec_n;
      asm volatile("" : "+s"(meta), "+s"(rec));  // (this op's words are in scalar registers from here on)
      {
        int64_t on = o + 1;
        if (on >= o1 && (!chained || on >= o_blk_end)) on = o;  // nothing follows (in this block's range of the stream): request this op again
        meta_n = sload_here<uint32_t>(ops.op_meta + on);
        rec_n = sload_here<u32x16>(ops.op_kfac + on * 8);
        __builtin_amdgcn_sched_barrier(0);
      }
      const uint32_t kind = meta & kOpKindMask;
      const int io = static_cast<int>((meta >> kOpIoShift) & kOpIoMask);
      auto rec_f64 = [&rec](int k) {
        return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(rec[2 * k + 1]) << 32) | rec[2 * k]));
      };
      const double a = rec_f64(7);
      const double* cov = ops.op_fac + o * (m.n_derived * PMX_MAX_FACTORS);  // (derived volumes: lane_out)
      if (kind == OP_PROP) {
        // bits 24-26: 0 = build; 1 + k = build and keep in slot k; 1 + S + k = take slot k (pmx_compile.cpp)
        const uint32_t rc = (meta >> kOpCacheShift) & kOpCacheMask;
        const uint32_t n_slots = static_cast<uint32_t>(prop_slots);
        double q[LM::NKP], keep[ND0];
        {
          double kp[LM::NKP];
#pragma unroll
          for (int j = 0; j < LM::NKP; ++j) kp[j] = L.kp_base[j] * rec_f64(j);
          to_native_params<KID>(kp, q);
        }
        if (rc > n_slots) {
#pragma unroll
          for (int k = 0; k < ND0; ++k) keep[k] = prop_cache[((rc - 1u - n_slots) * ND0 + k) * tile + threadIdx.x];
        } else {
          // bit 27: same covariate factor row as the occasion's previous built segment - its eigenvalues still hold
          bool ok;
          if constexpr (EIGR) {
            ok = (meta & kOpSameFacBit) ? LM::S::template direct0_make<true>(q, a, keep, lprev, okprev)
                                     : LM::S::template direct0_make<false>(q, a, keep, lprev, okprev);
          } else {
            ok = LM::S::template direct0_make<false>(q, a, keep, lprev, okprev);
          }
          if (!ok) st = PMX_PAIR_COMPLEX_ROOTS;
          if (rc != 0u) {
#pragma unroll
            for (int k = 0; k < ND0; ++k) prop_cache[((rc - 1u) * ND0 + k) * tile + threadIdx.x] = keep[k];
          }
        }
        LM::S::direct0_apply(q, keep, x);
      } else if (kind == OP_OBS) {
        double y = lane_out_uniform<KID>(m, L, x, io, cov);
        if (st == PMX_PAIR_COMPLEX_ROOTS) y = nanv;
        if constexpr (LL) {
          ll_accumulate(as_const(ops.ll_obs) + row * 4, y, ll_acc);
        } else {
          if (st == PMX_PAIR_OK && !isfinite(y)) st = PMX_PAIR_NONFINITE;
          if (lane_ok) pred[row * ld + p] = y;
        }
        ++row;
      } else if (kind == OP_BOLUS) {
        const double amt = a * fa_of(m, th, io);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] += (i == io) ? amt : 0.0;
      } else {  // OP_RESET
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = io ? L.xinit[i] : 0.0;
        if (st_sticky == PMX_PAIR_OK) st_sticky = st;
        st = PMX_PAIR_OK;
      }
    }
    if (st_sticky != PMX_PAIR_OK) st = st_sticky;
    if constexpr (LL) {
      if (st == PMX_PAIR_OK && !isfinite(ll_acc)) st = PMX_PAIR_NONFINITE;
      if (lane_ok) ops.ll_out[s * ops.ll_ld + p] = (st == PMX_PAIR_OK || st == PMX_PAIR_NONFINITE) ? ll_acc : nanv;
    }
    if (status != nullptr && lane_ok && (st != PMX_PAIR_OK || zero_status == 2)) {
      if (zero_status == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      status[s * P + p] = st;
    }
  }
}

}  // namespace

hipError_t launch_dyn3(const LaunchArgs& a, const Route& r) {
  if (!r.dyn || r.lag) return hipErrorInvalidValue;
  return with_kid(a.m.kernel, [&](auto kid) {
    if constexpr (kHasDirect0<kernel_structure(decltype(kid)::value)>) {
      return dispatch([&](auto ll, auto eigr) {
        hipLaunchKernelGGL((pmx_analytical_dyn3<decltype(kid)::value, decltype(ll)::value, decltype(eigr)::value>), dim3(static_cast<uint32_t>(r.blocks)), dim3(r.threads),
                           r.lds, static_cast<hipStream_t>(a.stream), a.m, a.ops, a.theta, a.P, r.n, r.s_chunk, r.n_ptiles, a.pred, a.ld,
                           a.status, r.leftover ? a.cls.generic_subjects : nullptr, a.cls.zero_status, a.prop_slots);
        return hipGetLastError();
      }, r.ll, r.eig_reuse);
    } else {
      return hipErrorInvalidValue;
    }
  });
}

}  // namespace pmx

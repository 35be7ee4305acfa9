// pmx_classed_ll.hip — the pipelined classed log-likelihood kernel (exact classes of plain models).
#include "pmx_lanes.hpp"

namespace pmx {

namespace {

// ------------------------------------------------------------------------------------
// CLASSED log-likelihood kernel, exact classes of plain models - the entry NPAG calls (log_likelihood_matrix,
// likelihood/matrix.rs:52-106).  Same arithmetic per (subject, support point) as pmx_analytical_classed<KID, true>; what
// is different is how a wave gets its scalars.  Stamped with s_memtime (tools/ll_stamps.py), the round-2 shape spent 46 %
// of its wave time in the chunk epilogue and 7 % in the chunk header - dependent scalar fetches of data that streams
// from HBM once (subject ids, offsets), one after the other, each a full memory latency - and waited on five scalar
// blocks at the top of every step.  Here
//   * everything a chunk needs is ONE 128-byte record (DevClassPlan::chunk_hdr: program, offsets, masks, the G subject
//     ids), requested a chunk ahead - at the start of the previous chunk's epilogue;
//   * a step's {meta, dt} is one 16-byte record, requested a step ahead; its observation block (G observed values + G
//     weights) one pair of wide fetches requested at the top of the step and first touched behind the state update
//     (volatile fetches pinned by scheduling barriers: the compiler sinks plain ones to their use);
//   * the members' constant sums are requested in front of the run that closes the chunk and added behind it;
//   * runs of steps that are on the exponential ladder, carry a row of output 0 and see no infusion in this chunk are
//     straight-line code (one basic block per step, every value updated in place); a missing observation's weight 0
//     makes its term vanish, so without censored rows (CENS = false) every row qualifies;
//   * a step in which no live member has an infusion running builds F only and advances with apply0;
//   * the lane's initial state and every other per-lane value is in registers before the chunk loop: no vector load
//     (and so no s_waitcnt vmcnt behind the previous chunk's stores) on the common path.
// ------------------------------------------------------------------------------------
#ifdef PMX_LL_STAMPS
__device__ uint64_t g_ll_stamps[5];  // diagnostic build only (tools/ll_stamps.py): cycles per phase, summed over waves
#endif
// Scalar fetches that stay where they are written.  Left to the compiler a request whose only use is the next trip of a
// loop sinks to the end of the trip, a dozen instructions in front of its wait; a VOLATILE fetch is not moved by the
// optimiser, and a scheduling barrier behind it keeps the instruction scheduler from moving it either.  (The waits are the
// compiler's own: it knows these registers are pending.  An earlier form issued the fetches from inline assembly - faster
// to write, but the register allocator may spill or copy an output it believes is already there.)
template <int G>
struct ObsRequest;
template <>
struct ObsRequest<8> {
  typedef u32x16 V;
};
template <>
struct ObsRequest<4> {
  typedef u32x8 V;
};

#ifndef PMX_LL_WAVES
#define PMX_LL_WAVES 3
#endif
template <int KID, bool CENS>
__global__ __launch_bounds__(kBlock, (LaneModel<KID>::NS <= 2) ? PMX_LL_WAVES : 2) void pmx_analytical_classed_ll(
    DevModel m, DevOps ops, DevClassPlan cp, const double* __restrict__ theta, int64_t P, int32_t n_ptiles,
    uint8_t* __restrict__ status) {
  using LM = LaneModel<KID>;
  constexpr int NS = LM::NS;
  constexpr int G = ClassBatch<KID>::G;
  using Req = ObsRequest<G>;
  const auto [ptile, cblock, n_cblocks] = classed_block(n_ptiles);
  const int64_t c_end = cp.n_chunks_exact;
  if (cblock >= c_end) return;
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t p = static_cast<int64_t>(ptile) * kBlock + threadIdx.x;
  const bool lane_ok = p < P;
  const int64_t pc = lane_ok ? p : (P - 1);
  const double* __restrict__ th = theta + pc * m.nparams;
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);

  typename LM::S::Coef coef;
  double inv_vol0;
  bool lane_good;
  double xinit[NS];  // (in registers for the whole launch: see the header comment)
  {
    LM L;
    lane_setup<KID, false>(m, th, L);
    coef = L.coef;
    lane_good = L.ok;
    inv_vol0 = L.ok ? L.inv_vol[0] : nanv;
#pragma unroll
    for (int i = 0; i < NS; ++i) xinit[i] = L.xinit[i];
  }
  const auto chunk_row = as_const(cp.chunk_row);
  const auto val = as_const(cp.val);
  const auto cobs = as_const(cp.cobs);
  (void)chunk_row;
  const int out_state0 = m.out[0].state - m.pm;
  const char* hdr_base = reinterpret_cast<const char*>(cp.chunk_hdr);
  // the lane's slot in its row of the output, ll_out[sid][p], and the row pitch in bytes - the pitch parked in a VECTOR
  // register: as a scalar it does not survive the register pressure of the step loop, and re-fetched from the kernel
  // arguments in front of every store (s_load + s_waitcnt, which also waits for the header request in flight) it made
  // the epilogue half of the wave's time (tools/ll_stamps.py)
  char* const ll_lane = reinterpret_cast<char*>(ops.ll_out + p);
  uint32_t ll_pitch = static_cast<uint32_t>(ops.ll_ld * 8);  // (host-checked: fits 32 bits)
  asm volatile("" : "+v"(ll_pitch));

#ifdef PMX_LL_STAMPS
  uint64_t tp[5] = {0, 0, 0, 0, 0};  // diagnostic build only: shader cycles per phase (header, slow steps, fast runs, epilogue, whole wave)
  const uint64_t t_wave0 = __builtin_amdgcn_s_memtime();
#define PMX_STAMP(i, t_prev)                              \
  {                                                       \
    const uint64_t t_now_ = __builtin_amdgcn_s_memtime(); \
    tp[i] += t_now_ - t_prev;                             \
    t_prev = t_now_;                                      \
  }
#else
#define PMX_STAMP(i, t_prev)
#endif

  // the NEXT chunk's header record, requested a chunk ahead
  u32x16 h_n = sload_here<u32x16>(hdr_base + cblock * 64);
  for (int64_t c = cblock; c < c_end; c += n_cblocks) {
#ifdef PMX_LL_STAMPS
    uint64_t t_ph = __builtin_amdgcn_s_memtime();
#endif
    u32x16 h = h_n;
    asm volatile("" : "+s"(h));
    // {n_live | n_steps << 16, program offset, val offset, cobs offset, rate mask, class fast mask, subject ids}
    const int32_t n_live = static_cast<int32_t>(h[0] & 0xffffu);
    const int32_t n_steps = static_cast<int32_t>(h[0] >> 16);
    const int64_t pb = static_cast<int64_t>(h[1]);
    int64_t voff = static_cast<int64_t>(h[2]);
    const int64_t cbase = static_cast<int64_t>(h[3]);
    const uint64_t rate_mask = (static_cast<uint64_t>(h[5]) << 32) | h[4];
    uint64_t fast_mask = ((static_cast<uint64_t>(h[7]) << 32) | h[6]) & ~rate_mask & 0x7fffffffffffffffull;
    // the G subject ids wait for the epilogue in ONE vector register (lane j holds member j's): eight scalar registers
    // less across the step loop, whose straight-line runs hold two observation blocks at a time
    int32_t sid_park = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) sid_park = (static_cast<int>(lane) == j) ? static_cast<int32_t>(h[8 + j]) : sid_park;
    int64_t cobs_off = cbase + 2 * G;  // (behind the chunk's [G] constant sums and [G] flags)
    if constexpr (CENS) {
      // censored / residual-model rows take the general fold: only the steps whose row is plain for every live member
      // (the mask by program step, pmx_ll_prepare_chunks) run straight-line.  (a dependent fetch: this variant is the rare one)
      fast_mask &= static_cast<uint64_t>(__double_as_longlong(cobs[cbase + G + 1]));
    }
    if (cp.zero_status == 1 && status != nullptr) {  // (see pmx_analytical_classed)
      const int zj = static_cast<int>(lane >> 3);
      int64_t zsid = -1;
#pragma unroll
      for (int j = 0; j < G; ++j) zsid = (zj == j && j < n_live) ? static_cast<int64_t>(static_cast<int32_t>(h[8 + j])) : zsid;
      const int64_t zp = static_cast<int64_t>(ptile) * kBlock + (threadIdx.x & ~63u) + 8 * (lane & 7u);
      if (zsid >= 0 && zp < P) *reinterpret_cast<uint64_t*>(status + zsid * P + zp) = 0ull;
    }
    double ll_acc[G], x[G][NS];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      ll_acc[j] = 0.0;
#pragma unroll
      for (int i = 0; i < NS; ++i) x[j][i] = 0.0;
    }
    uint32_t bad = 0;
    double ex[LM::S::NE];
#pragma unroll
    for (int i = 0; i < LM::S::NE; ++i) ex[i] = 0.0;
    int32_t kobs = 0;
    bool csum_in = false;  // the members' constant sums (the block behind the chunk's last observation block) are in the sums
    const double* recs = cp.prog_rec + 2 * pb;
    int32_t k = 0;
    PMX_STAMP(0, t_ph)
    while (k < n_steps) {
      const uint64_t run_bits = (k < 63) ? (fast_mask >> k) : 0ull;
      if (run_bits & 1ull) {
        // ---- a run of straight-line steps: x' = F x, fold the row.  The output's state is picked OUTSIDE the loop (one
        // copy of the loop per state) and the ladder is a one-sided branch, so a step is straight-line code that updates
        // every value in place; the record of the NEXT step and its observation block are requested at the step's top.
        int32_t run = __builtin_ctzll(~run_bits);
        if (run > n_steps - k) run = n_steps - k;
        const bool closes = (k + run == n_steps);  // this run holds the chunk's last step
        auto fast_run = [&](auto st_c) {
          constexpr int ST = decltype(st_c)::value;
          // the members' constant sums (head of the chunk's block) ride along when this run closes the chunk: requested
          // here, added behind the loop
          typename Req::V cs_v;
          if (closes) cs_v = sload_here<typename Req::V>(cp.cobs + cbase);
          uint64_t w_n = sload_here<uint64_t>(recs + 2 * k);
#pragma unroll 1
          for (int32_t i = 0; i < run; ++i) {
            // this step's observation block goes out at the top of the step and is first touched behind the state update
            // (keeping TWO blocks in flight - a whole step ahead - cost 32 more scalar registers and the spills that came
            // with them: 0.53 ms against 0.48 on C3); the next step's record goes out a step ahead
            uint64_t w = w_n;
            asm volatile("" : "+s"(w));
            const typename Req::V yc = sload_here<typename Req::V>(cp.cobs + cobs_off);
            const typename Req::V wc = sload_here<typename Req::V>(cp.cobs + cobs_off + G);
            w_n = sload_here<uint64_t>(recs + 2 * (k + i + 1));  // (behind the last program record: one record of padding)
            __builtin_amdgcn_sched_barrier(0);
            cobs_off += 2 * G;
            double ov_y[G], ov_w[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
              ov_y[j] = __longlong_as_double(static_cast<int64_t>((static_cast<uint64_t>(yc[2 * j + 1]) << 32) | yc[2 * j]));
              ov_w[j] = __longlong_as_double(static_cast<int64_t>((static_cast<uint64_t>(wc[2 * j + 1]) << 32) | wc[2 * j]));
            }
            const uint32_t rung = (static_cast<uint32_t>(w) >> kOpRungShift) & kOpRungMask;  // 1..4
            if (rung != 1u) {
#pragma unroll
              for (int e = 0; e < LM::S::NE; ++e) {
                const double bse = ex[e];
                const double sq = bse * bse;
                double r = sq;
                if (rung != 2u) r = sq * ((rung == 3u) ? bse : sq);
                ex[e] = r;
              }
            }
            typename LM::S::Prop pr;
            LM::S::from_exps_f(coef, ex, pr);
#pragma unroll
            for (int j = 0; j < G; ++j) LM::S::apply0(pr, x[j]);
#pragma unroll
            for (int j = 0; j < G; ++j) {
              const double d = fma(-inv_vol0, x[j][ST], ov_y[j]);
              ll_acc[j] = fma(-(d * ov_w[j]), d, ll_acc[j]);  // (weight 0 = a missing observation: the term vanishes)
            }
          }
          if (closes) {
#pragma unroll
            for (int j = 0; j < G; ++j)
              ll_acc[j] += __longlong_as_double(static_cast<int64_t>((static_cast<uint64_t>(cs_v[2 * j + 1]) << 32) | cs_v[2 * j]));
          }
        };
        if (out_state0 == 0) fast_run(std::integral_constant<int, 0>{});
        if constexpr (NS > 1) {
          if (out_state0 == 1) fast_run(std::integral_constant<int, 1>{});
        }
        if constexpr (NS > 2) {
          if (out_state0 == 2) fast_run(std::integral_constant<int, 2>{});
        }
        if constexpr (NS > 3) {
          if (out_state0 == 3) fast_run(std::integral_constant<int, 3>{});
        }
        kobs += run;
        voff += static_cast<int64_t>(run) * G;
        k += run;
        csum_in = closes;
        PMX_STAMP(2, t_ph)
        continue;
      }
      // ---- any other step: the general form
      const auto rp = as_const(reinterpret_cast<const uint64_t*>(recs)) + 2 * k;
      const uint64_t w = rp[0], dtb = rp[1];
      const uint32_t meta = static_cast<uint32_t>(w);
      const uint32_t kind = meta & kOpKindMask;
      const int io = static_cast<int>((meta >> kOpIoShift) & kOpIoMask);
      const bool has_val = ((rate_mask >> (k < 63 ? k : 63)) & 1ull) != 0ull;
      if (kind == OP_PROP) {
        const uint32_t rung = (meta >> kOpRungShift) & kOpRungMask;
        if (rung == 0u) {
          LM::S::exps(coef, __longlong_as_double(static_cast<int64_t>(dtb)), ex);
        } else if (rung != 1u) {
          ladder_pow<LM::S::NE>(ex, rung);
        }
        typename LM::S::Prop pr;
        LM::S::from_exps_f(coef, ex, pr);
#pragma unroll
        for (int j = 0; j < G; ++j) LM::S::apply0(pr, x[j]);
        if (has_val) {  // wave-uniform: somebody infuses - the response to the members' rates on top
          LM::S::from_exps_j(coef, ex, pr);
#pragma unroll
          for (int j = 0; j < G; ++j) LM::S::add_j(pr, x[j], val[voff + j]);
        }
      } else if (kind == OP_BOLUS) {
        double f = fa_of(m, th, io);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(f)::"memory");  // (the lane's fa is consumed HERE, not behind the join)
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const double a = val[voff + j] * f;
#pragma unroll
          for (int i = 0; i < NS; ++i) x[j][i] += (i == io - m.pm) ? a : 0.0;
        }
      } else if (kind == OP_RESET) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          const double xi = io ? xinit[i] : 0.0;
#pragma unroll
          for (int j = 0; j < G; ++j) x[j][i] = xi;
        }
      }
      if ((meta >> kOpObsAfterShift) & 1u) {  // the observation fused into this step
        const auto ov = cobs + cobs_off;
        double ov_y[G], ov_w[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
          ov_y[j] = ov[j];
          ov_w[j] = ov[G + j];
        }
        const int oq = static_cast<int>((meta >> kOpOutShift) & kOpOutMask);
        int out_state = out_state0;
        double inv_vol = inv_vol0;
        if (oq != 0) {  // outputs beyond the first: rare (see pmx_analytical_classed for why it is written this way)
          out_state = m.out[oq].state - m.pm;
          const int vp = m.out_vol_theta[oq];
          double v = 1.0;
          if (vp >= 0) v = th[vp];
          double iv = 1.0 / v;
          asm volatile("" : "+v"(iv));
          inv_vol = lane_good ? iv : nanv;
        }
        auto fold = [&](auto st_c) {
          constexpr int ST = decltype(st_c)::value;
#pragma unroll
          for (int j = 0; j < G; ++j) {
            const int64_t wb = __double_as_longlong(ov_w[j]);
            if (wb != 0) {  // wave-uniform; weight 0 = missing observation (or chunk padding)
              if (CENS && wb < 0) {  // censored / residual-model row: the generic fold on its full record
                ll_accumulate(as_const(ops.ll_obs) + (chunk_row[c * G + j] + kobs) * 4, x[j][ST] * inv_vol, ll_acc[j]);
              } else {
                const double d = fma(-inv_vol, x[j][ST], ov_y[j]);
                ll_acc[j] = fma(-(d * ov_w[j]), d, ll_acc[j]);
              }
            }
          }
        };
        if (out_state == 0) fold(std::integral_constant<int, 0>{});
        if constexpr (NS > 1) {
          if (out_state == 1) fold(std::integral_constant<int, 1>{});
        }
        if constexpr (NS > 2) {
          if (out_state == 2) fold(std::integral_constant<int, 2>{});
        }
        if constexpr (NS > 3) {
          if (out_state == 3) fold(std::integral_constant<int, 3>{});
        }
        cobs_off += 2 * G;
        ++kobs;
      }
      voff += G;
      ++k;
      PMX_STAMP(1, t_ph)
    }
    // ---- epilogue.  The next chunk's header goes out first: the stores below cover its fetch.
    {
      const int64_t c_next = (c + n_cblocks < c_end) ? (c + n_cblocks) : c;
      h_n = sload_here<u32x16>(hdr_base + c_next * 64);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!csum_in) {  // (the chunk ended in a general step: fetch the constant sums now)
      const auto cs = cobs + cbase;
#pragma unroll
      for (int j = 0; j < G; ++j) ll_acc[j] += cs[j];
    }
    double nanacc = 0.0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (j < n_live) {  // wave-uniform
        const double llj = ll_acc[j];
        nanacc = fma(llj, 0.0, nanacc);  // 0 * v is NaN iff v is not finite: resolved to members only in the rare wave that saw one
        const uint32_t sidj = static_cast<uint32_t>(__builtin_amdgcn_readlane(sid_park, j));
        double* const dst = reinterpret_cast<double*>(ll_lane + static_cast<uint64_t>(sidj) * ll_pitch);  // one v_mad_u64_u32
        // streaming store: the matrix is written once and read by nobody on this device (plain stores, which allocate in L2:
        // 0.600 ms on C3; nt: 0.530 - the wave sat in front of its eight stores for half its time, tools/ll_stamps.py)
        if (lane_ok) __builtin_nontemporal_store(llj, dst);  // (NaN already for a lane with complex roots)
      }
    }
    if (status != nullptr) {
      if (__any((nanacc != nanacc) ? 1 : 0)) {  // NonFiniteLikelihood (prediction.rs:119-124)
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (j < n_live && !isfinite(ll_acc[j])) bad |= (1u << j);
      }
      if (cp.zero_status == 2 || __any(((bad != 0u || !lane_good) && lane_ok) ? 1 : 0)) {
        if (cp.zero_status == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clearing store above lands first
#pragma unroll
        for (int j = 0; j < G; ++j) {
          if (j < n_live) {
            const uint8_t st = !lane_good ? PMX_PAIR_COMPLEX_ROOTS : (((bad >> j) & 1u) ? PMX_PAIR_NONFINITE : PMX_PAIR_OK);
            if (lane_ok && (st != PMX_PAIR_OK || cp.zero_status == 2))
              status[static_cast<int64_t>(__builtin_amdgcn_readlane(sid_park, j)) * P + p] = st;
          }
        }
      }
    }
    PMX_STAMP(3, t_ph)
  }
#ifdef PMX_LL_STAMPS
  tp[4] = __builtin_amdgcn_s_memtime() - t_wave0;
  if ((threadIdx.x & 63u) == 0u)
    for (int i = 0; i < 5; ++i) atomicAdd(reinterpret_cast<unsigned long long*>(&g_ll_stamps[i]), static_cast<unsigned long long>(tp[i]));
#endif
#undef PMX_STAMP
}


}  // namespace

hipError_t launch_classed_ll(const LaunchArgs& a, const Route& r) {
  if (r.dyn || r.lag) return hipErrorInvalidValue;  // (exact classes of plain models only)
  return with_kid(a.m.kernel, [&](auto kid) {
    return dispatch([&](auto cens) {
      hipLaunchKernelGGL((pmx_analytical_classed_ll<decltype(kid)::value, decltype(cens)::value>), dim3(static_cast<uint32_t>(r.blocks)),
                         dim3(r.threads), 0, static_cast<hipStream_t>(a.stream), a.m, a.ops, a.cls, a.theta, a.P, r.n_ptiles, a.status);
      return hipGetLastError();
    }, r.cens);
  });
}

#ifdef PMX_LL_STAMPS
}  // namespace pmx
extern "C" int32_t pmx_debug_ll_stamps(uint64_t* out5, int32_t reset) {  // diagnostic build only
  uint64_t z[5] = {0, 0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (out5 && hipMemcpyFromSymbol(out5, HIP_SYMBOL(pmx::g_ll_stamps), sizeof(z)) != hipSuccess) return 2;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(pmx::g_ll_stamps), z, sizeof(z)) != hipSuccess) return 3;
  return 0;
}
namespace pmx {
#endif

}  // namespace pmx

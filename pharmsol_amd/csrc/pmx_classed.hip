// pmx_classed.hip — the classed GRID kernel: G subjects of one class per lane, predictions or log-likelihood.
#include "pmx_lanes.hpp"

namespace pmx {

namespace {

// ------------------------------------------------------------------------------------
// CLASSED GRID kernel (analytical): one propagator per (lane, program step), applied to a
// register-resident batch of G subjects that share a dosing/sampling design (pmx_compile.hpp
// ClassPlan).  Per (subject, support point) the arithmetic is the generic kernel's; what goes away
// is recomputing exp(-lambda*dt) for every member, and fetching/decoding the op stream per subject.
// ------------------------------------------------------------------------------------
// Emit one observation row for every member of the chunk: y = x[ST] * inv_vol, stored in PAIRS.
// Lanes 0-31 of a wave own the even support points of the wave's 64, lanes 32-63 the odd ones; one
// v_permlane32_swap per dword turns (member A value, member B value) into (two adjacent doubles of A's
// row | two adjacent doubles of B's row), so a pair of members leaves in ONE 16-byte store per lane.
// `slot[h]` is this lane's 16-byte slot in the first prediction row of pair h (lower half-wave: member
// 2h, upper half-wave: member 2h+1).  Non-finite predictions are caught with one FMA per value
// (0*y is NaN iff y is inf/NaN) and resolved to members only in the rare wave that saw one.
template <int ST, int G, int NS>
__device__ __forceinline__ void classed_emit(const double (&x)[G][NS], double inv_vol, double* const (&slot)[G / 2],
                                             int64_t kld, bool upper, bool pair_full, bool pair_half, bool any_half,
                                             int32_t n_live, uint32_t& bad) {
  double nanacc = 0.0;
#pragma unroll
  for (int h = 0; h < G / 2; ++h) {
    if (2 * h < n_live) {  // wave-uniform
      const double ya = x[2 * h][ST] * inv_vol;
      const double yb = x[2 * h + 1][ST] * inv_vol;
      nanacc = fma(ya, 0.0, nanacc);
      nanacc = fma(yb, 0.0, nanacc);
      uint32_t alo = static_cast<uint32_t>(__double_as_longlong(ya));
      uint32_t ahi = static_cast<uint32_t>(static_cast<uint64_t>(__double_as_longlong(ya)) >> 32);
      uint32_t blo = static_cast<uint32_t>(__double_as_longlong(yb));
      uint32_t bhi = static_cast<uint32_t>(static_cast<uint64_t>(__double_as_longlong(yb)) >> 32);
      const auto r0 = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
      const auto r1 = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
      double2 v;
      v.x = __longlong_as_double(static_cast<int64_t>((static_cast<uint64_t>(r1[0]) << 32) | r0[0]));
      v.y = __longlong_as_double(static_cast<int64_t>((static_cast<uint64_t>(r1[1]) << 32) | r0[1]));
      const bool row_live = (2 * h + 1 < n_live) || !upper;  // the last pair of a partial chunk has no member B
      double* dst = slot[h] + kld;
      if (row_live && pair_full) {
        typedef double dbl2 __attribute__((ext_vector_type(2)));
        dbl2 vv;
        vv.x = v.x;
        vv.y = v.y;
        // streaming store, cache policy `sc1 nt` (tools/experiments/store_pattern_probe.hip: plain 1.23 ms, nt 1.12, sc1 nt 1.07
        // for this address map); no builtin carries sc1, hence the asm
        asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(dst), "v"(vv) : "memory");
      }
      if (any_half) {  // wave-uniform: only the wave holding the last slot of an odd-length row
        if (row_live && pair_half) *dst = v.x;
      }
    }
  }
  if (__any((nanacc != nanacc) ? 1 : 0)) {  // rare: find out which members
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j < n_live && !isfinite(x[j][ST] * inv_vol)) bad |= (1u << j);
  }
}

template <int ST, int G, int NS>
__device__ __forceinline__ void classed_emit_state(int out_state, const double (&x)[G][NS], double inv_vol,
                                                   double* const (&slot)[G / 2], int64_t kld, bool upper, bool pair_full,
                                                   bool pair_half, bool any_half, int32_t n_live, uint32_t& bad) {
  if (out_state == ST) {
    classed_emit<ST, G, NS>(x, inv_vol, slot, kld, upper, pair_full, pair_half, any_half, n_live, bad);
  } else if constexpr (ST + 1 < NS) {
    classed_emit_state<ST + 1, G, NS>(out_state, x, inv_vol, slot, kld, upper, pair_full, pair_half, any_half, n_live,
                                      bad);
  }
}

// __launch_bounds__ 2nd argument = waves per SIMD the register allocator must leave room for
// (4 -> at most 128 VGPRs): the kernel is a latency/bandwidth mix and wants the occupancy.
// LAGC: one lagged input (exact classes only).  The members of a class share every bolus TIME, so a lane's lagged
// landing times t + lag(theta) - its split points inside a PROP step - are the same for all G members: one propagator
// per sub-interval still serves the whole batch; only the amounts are the members' own (lag_prop / lag_open_occasion
// of the generic walker, over G states at once).
// CENS (log-likelihood mode): the population holds censored observations; their rows are marked in the chunk blocks
// and folded from their full records (a separate instantiation: the extra branch costs the uncensored kernel 9 %).
// DYNC (with PERDT): covariate-derived rate constants / volumes.  The members share the program shape only; each
// rebuilds its propagator from its own covariate factors (the generic walker's lane_advance_dyn, the plan's facp
// rows) and scales its output by its own volume (lane_out, faco rows).  Complex roots are a member's, per occasion.
template <int KID, bool LL, bool PERDT, bool LAGC = false, bool CENS = false, bool DYNC = false>
__global__ __launch_bounds__(kBlock, (LaneModel<KID>::NS <= 2) ? 4 : 2) void pmx_analytical_classed(
    DevModel m, DevOps ops, DevClassPlan cp, const double* __restrict__ theta, int64_t P, int32_t chunks_per_block,
    int32_t n_ptiles, double* __restrict__ pred, int64_t ld, uint8_t* __restrict__ status) {
  using LM = LaneModel<KID>;
  constexpr int NS = LM::NS;
  constexpr int G = ClassBatch<KID>::G;
  static_assert(G % 2 == 0, "members are stored in pairs");
  const auto [ptile, cblock, n_cblocks] = classed_block(n_ptiles);
  // this launch's share of the plan: the chunks with shared step lengths, or (PERDT) the loose ones behind them
  const int64_t c_begin = PERDT ? cp.n_chunks_exact : 0;
  const int64_t c_end = PERDT ? cp.n_chunks : cp.n_chunks_exact;
  if (c_begin + cblock >= c_end) return;
  const uint32_t lane = threadIdx.x & 63u;
  const bool upper = lane >= 32u;
  const int64_t p_even = static_cast<int64_t>(ptile) * kBlock + (threadIdx.x & ~63u) + 2u * (lane & 31u);
  const int64_t p = p_even + (upper ? 1 : 0);
  const bool lane_ok = p < P;
  const int64_t pc = lane_ok ? p : (P - 1);
  const bool pair_full = (p_even + 1) < P;   // this lane's 16-byte slot [p_even, p_even+1] is inside the row
  const bool pair_half = (p_even + 1) == P;  // only its first 8 bytes are (odd n_support, last slot of a row)
  const bool any_half = __any(pair_half ? 1 : 0) != 0;

  typename LM::S::Coef coef;
  // 1/volume of output 0.  A lane with complex roots has NaN coefficients (lane_setup): its rows are NaN from an occasion's
  // first PROP on, like every walker's.  Its log-likelihood sum is NaN as a whole (a failed pair has no sum), and every
  // class program propagates (pmx_plan.cpp build_class_plan), so the pair is PMX_PAIR_COMPLEX_ROOTS.
  double inv_vol0;
  bool lane_good;
  LM Ld;  // DYNC: the lane's base parameters, kept for the per-member rebuilds
  if constexpr (DYNC) {
    lane_setup<KID, true>(m, theta + pc * m.nparams, Ld);
    lane_good = true;
    inv_vol0 = Ld.inv_vol[0];
  } else {
    LM L;
    lane_setup<KID, false>(m, theta + pc * m.nparams, L);
    coef = L.coef;
    lane_good = L.ok;
    inv_vol0 = (L.ok || !LL) ? L.inv_vol[0] : __longlong_as_double(0x7ff8000000000000LL);
  }
  (void)Ld;
  double lagv = 0.0;      // LAGC: this lane's lag time of the lagged input
  bool lane_badlag = false;
  if constexpr (LAGC) {
    lagv = theta[pc * m.nparams + m.lag_param[0]];
    if (lagv != lagv) {  // NaN lag: PMX_PAIR_BAD_LAG, rows NaN (the generic walker's rule; a negative lag is a shift to earlier)
      lane_badlag = true;
      inv_vol0 = __longlong_as_double(0x7ff8000000000000LL);
    }
  }
  const double kInf = __longlong_as_double(0x7ff0000000000000LL);
  (void)kInf;
  // the plan arrays are read-only for the whole launch and every index below is wave-uniform:
  // constant-address-space pointers make these scalar (s_load) fetches
  const auto prog_meta = as_const(cp.prog_meta);
  const auto prog_dt = as_const(cp.prog_dt);
  const auto cls_prog_off = as_const(cp.cls_prog_off);
  const auto chunk_cls = as_const(cp.chunk_cls);
  const auto chunk_n = as_const(cp.chunk_n);
  const auto chunk_val_off = as_const(cp.chunk_val_off);
  const auto chunk_subj = as_const(cp.chunk_subj);
  const auto chunk_row = as_const(cp.chunk_row);
  const auto val = as_const(cp.val);
  const auto dtv = as_const(cp.dtv);
  (void)dtv;
  const double* __restrict__ th = theta + pc * m.nparams;

  (void)chunks_per_block;
  for (int64_t c = c_begin + cblock; c < c_end; c += n_cblocks) {
    const int32_t cls = chunk_cls[c];
    const int32_t n_live = chunk_n[c];
    int64_t voff = chunk_val_off[c];
    const int64_t pb = cls_prog_off[cls];
    const int64_t pe = cls_prog_off[cls + 1];
    int64_t kld = 0;   // (observations emitted so far) * ld
    if (cp.zero_status == 1 && status != nullptr) {
      // The wave clears the status bytes it owns (G members x its 64 support points) with ONE 8-byte store per lane:
      // lane = 8 * member + piece.  A separate memset between two passes cost ~70 us of serialisation per pass, this
      // costs one store per chunk.  (Launcher guarantees n_support % 8 == 0 and G <= 8 when the flag is set.)
      const int zj = static_cast<int>(lane >> 3);
      int64_t zsid = -1;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int64_t sj = chunk_subj[c * G + j];
        zsid = (zj == j && j < n_live) ? sj : zsid;
      }
      const int64_t zp = static_cast<int64_t>(ptile) * kBlock + (threadIdx.x & ~63u) + 8 * (lane & 7u);
      if (zsid >= 0 && zp < P) *reinterpret_cast<uint64_t*>(status + zsid * P + zp) = 0ull;
    }
    uint64_t plain_obs = 0;  // log-likelihood mode: bit k = observation k is a plain row for every live member
    (void)plain_obs;
    double* slot[G / 2];  // this lane's 16-byte slot in the first prediction row of each member pair
    double ll_acc[G];     // log-likelihood mode: running sum of each member
    int64_t cobs_off = 0;  // log-likelihood mode: the chunk's {value, const, weight} block, advanced per observation
    int64_t kobs = 0;      // ... and how many observations of the program have been folded
    (void)kobs;
    if constexpr (LL) {
      cobs_off = as_const(cp.chunk_obs_off)[c] + 2 * G;  // (behind the chunk's [G] constant sums and [G] flags)
      plain_obs = static_cast<uint64_t>(__double_as_longlong(as_const(cp.cobs)[cobs_off - G]));
#pragma unroll
      for (int j = 0; j < G; ++j) ll_acc[j] = 0.0;
    } else {
      const auto rows = chunk_row + c * G;
#pragma unroll
      for (int h = 0; h < G / 2; ++h) {
        int64_t ra = rows[2 * h] * ld, rb = rows[2 * h + 1] * ld;
        asm volatile("" : "+s"(ra), "+s"(rb));  // (keeps LLVM from selecting between the two ADDRESSES)
        slot[h] = pred + ((upper ? rb : ra) + p_even);
      }
    }
    double x[G][NS];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int i = 0; i < NS; ++i) x[j][i] = 0.0;
    uint32_t bad = 0;  // bit j: member j emitted a non-finite prediction
    uint32_t cplx = 0;  // DYNC: bit j: a rebuild of member j found complex eigenvalues in the current occasion
    uint32_t cplx_any = 0, bad_any = 0;  // DYNC: ... in an earlier occasion (status is sticky, the rows are not)
    (void)cplx;
    (void)cplx_any;
    (void)bad_any;
    // the lane's exponentials outlive a step: bits 27-29 of a PROP step say how this step's length relates
    // to the previous PROP's (0 = unrelated: exp(); 1 = equal; n = 2..4: n times as long: ladder_pow)
    double ex[LM::S::NE];
    // LAGC: cursor into the current occasion's list of lagged boluses (relative: the members' lists run in parallel),
    // the list's length and member 0's list (the shared times); reset_voff = the val row with the members' occasions
    int32_t lcur = 0, lcnt = 0;
    int64_t lbase0 = 0, reset_voff = 0;
    // every member advances by dt (per lane) under its own rate / takes its own amount of the lagged bolus at lcur
    auto advance_all = [&](double dt, int64_t rate_off, bool with_rate) {
      typename LM::S::Prop pr;
      make_prop<LM::ST>(coef, dt, pr);
#pragma unroll
      for (int j = 0; j < G; ++j) LM::S::apply(pr, x[j], with_rate ? val[rate_off + j] : 0.0);
    };
    auto bolus_all = [&]() {
      const double f = fa_of(m, th, m.lag_input[0]);
      const int dest = m.lag_dest[0];
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int64_t occ = static_cast<int64_t>(val[reset_voff + j]);  // (padding members: occasion 0, amounts unused)
        const double amt = ops.lagb_amount[as_const(ops.lagb_off)[occ] + lcur] * f;
#pragma unroll
        for (int i = 0; i < NS; ++i) x[j][i] += (i == dest) ? amt : 0.0;
      }
      ++lcur;
    };
    auto lag_tau = [&]() { return (lcur < lcnt) ? (ops.lagb_time[lbase0 + lcur] + lagv) : kInf; };
    (void)advance_all;
    (void)bolus_all;
    (void)lag_tau;
    for (int64_t o = pb; o < pe; ++o, voff += G) {
      const uint32_t meta = prog_meta[o];
      // Log-likelihood mode stores nothing inside this loop; what it waits for is scalar fetches, and fetched where they
      // are used a step has four of them one behind the other (meta -> lengths / rates -> descriptor -> observed values
      // and weights; SQ_WAIT_ANY: ~2000 cycles per wave-step).  So every scalar of the step is requested here, in one go,
      // whether or not the step turns out to need it (a step without an observation reads the next one's values; the
      // chunk's block is followed by the next chunk's, the array by 2 G doubles of slack), and pinned, so that the
      // compiler neither sinks the fetches back to their uses nor splits the wait.
      constexpr bool kUpfront = LL && !LAGC && !DYNC && !PERDT;
      double up_dt = 0.0, up_v[G], up_l[G], up_y[G], up_w[G];
      (void)up_dt;
      (void)up_v;
      (void)up_l;
      (void)up_y;
      (void)up_w;
      if constexpr (kUpfront) {
        const auto ov = as_const(cp.cobs) + cobs_off;
        if constexpr (!PERDT) up_dt = prog_dt[o];
#pragma unroll
        for (int j = 0; j < G; ++j) {
          up_v[j] = val[voff + j];
          if constexpr (PERDT) up_l[j] = dtv[voff + j];
          up_y[j] = ov[j];
          up_w[j] = ov[G + j];
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
          int64_t bv = __double_as_longlong(up_v[j]), by = __double_as_longlong(up_y[j]), bw = __double_as_longlong(up_w[j]);
          asm volatile("" : "+s"(bv), "+s"(by), "+s"(bw));
          up_v[j] = __longlong_as_double(bv);
          up_y[j] = __longlong_as_double(by);
          up_w[j] = __longlong_as_double(bw);
          if constexpr (PERDT) {
            int64_t bl = __double_as_longlong(up_l[j]);
            asm volatile("" : "+s"(bl));
            up_l[j] = __longlong_as_double(bl);
          }
        }
      }
      const uint32_t kind = meta & kOpKindMask;
      const int io = static_cast<int>((meta >> kOpIoShift) & kOpIoMask);
      if (kind == OP_PROP) {
        if constexpr (LAGC) {
          // lag_prop: split [t0, t1) at this lane's lagged landing times
          const double t1 = as_const(cp.prog_t1)[o];
          double t = as_const(cp.prog_t0)[o];
          for (;;) {
            const double tau = lag_tau();
            if (!(tau < t1)) break;
            if (tau > t) {
              advance_all(tau - t, voff, true);
              t = tau;
            }
            bolus_all();
          }
          if (t1 > t) advance_all(t1 - t, voff, true);
        } else if constexpr (DYNC) {
          const int64_t nf = cp.n_fac;
#pragma unroll
          for (int j = 0; j < G; ++j) {
            if (!lane_advance_dyn<KID, true>(m, Ld, cp.facp + (voff + j) * nf, x[j], dtv[voff + j], val[voff + j])) cplx |= (1u << j);
            if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);
          }
        } else if constexpr (PERDT) {
          // loose chunk: every member has its own step length, hence its own propagator; the members still share
          // the walk through the program (one scalar decode per step instead of G) and the paired stores
          // the step's 2 G scalars (lengths, rates) come in up front with two wide scalar loads: fetched member by member
          // each of the G blocks below began by waiting for its own s_load
          double m_dt[G], m_r[G];
#pragma unroll
          for (int j = 0; j < G; ++j) {
            m_dt[j] = kUpfront ? up_l[j] : dtv[voff + j];
            m_r[j] = kUpfront ? up_v[j] : val[voff + j];
          }
#pragma unroll
          for (int j = 0; j < G; ++j) {
            LM::S::exps(coef, m_dt[j], ex);
            step_from_exps<LM::ST>(coef, ex, x[j], m_r[j]);  // (the member's rate is a scalar: no infusion, no J)
            if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          const uint32_t rung = (meta >> kOpRungShift) & kOpRungMask;
          if (rung == 0u) {
            LM::S::exps(coef, kUpfront ? up_dt : prog_dt[o], ex);
          } else if (rung != 1u) {
            ladder_pow<LM::S::NE>(ex, rung);
          }
          typename LM::S::Prop pr;
          LM::S::from_exps(coef, ex, pr);  // (one propagator per step for G members: splitting off J does not pay here)
#pragma unroll
          for (int j = 0; j < G; ++j) {
            LM::S::apply(pr, x[j], kUpfront ? up_v[j] : val[voff + j]);
            // keep the scheduler from interleaving all G updates (it would hold old and new state of
            // every member at once: +2*NS*G registers, one wave per SIMD less)
            if ((j & 1) == 1) __builtin_amdgcn_sched_barrier(0);
          }
        }
      } else if (kind == OP_BOLUS) {
        const double f = fa_of(m, th, io);  // the lane's bioavailability of this input (1.0 when the model has none)
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const double a = (kUpfront ? up_v[j] : val[voff + j]) * f;
#pragma unroll
          for (int i = 0; i < NS; ++i) x[j][i] += (i == io - m.pm) ? a : 0.0;  // (pm_: model input 1 = kernel state 0)
        }
      } else if (kind == OP_RESET) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
          double xi = 0.0;
          if (io && m.has_init && m.init_param[i + m.pm] >= 0) xi = th[m.init_param[i + m.pm]];
          if constexpr (DYNC) {  // a new occasion re-derives its coefficients: its rows are finite again, but the pair
            cplx_any |= cplx;    // stays failed (the reference errors out for the whole subject)
            bad_any |= bad;
            cplx = 0;
            bad = 0;
          }
#pragma unroll
          for (int j = 0; j < G; ++j) x[j][i] = xi;
        }
        if constexpr (LAGC) {
          // lag_open_occasion: point the cursor at this occasion's list, run the boluses that land before the
          // occasion's first remaining event (no infusion can be active there)
          reset_voff = voff;
          const int64_t occ0 = static_cast<int64_t>(val[voff]);
          lbase0 = as_const(ops.lagb_off)[occ0];
          lcnt = static_cast<int32_t>(as_const(ops.lagb_off)[occ0 + 1] - lbase0);
          lcur = 0;
          const double t_first = as_const(cp.prog_t0)[o];
          bool started = false;
          double t = 0.0;
          for (;;) {
            const double tau = lag_tau();
            if (!(tau < t_first)) break;
            if (started && tau > t) advance_all(tau - t, voff, false);
            t = tau;
            started = true;
            bolus_all();
          }
          if (started && t_first > t && t_first < kInf) advance_all(t_first - t, voff, false);
        }
      }  // (kind == OP_OBS: a second observation at the same instant, no state change)
      if ((meta >> kOpObsAfterShift) & 1u) {  // the observation fused into this step (pmx_plan.cpp build_class_plan)
        if constexpr (LAGC) {
          // no PROP step in front of this observation (bit 31; its time sits in the step's t1 slot): the lagged boluses
          // landing before it come first, without propagation (the members share the landing times)
          if (meta >> kOpFlushShift) {
            const double t_obs = as_const(cp.prog_t1)[o];
            while (lag_tau() < t_obs) bolus_all();
          }
        }
        const int oq = static_cast<int>((meta >> kOpOutShift) & kOpOutMask);
        // (pm_ models: the plan only holds subjects that never dose the pad slot and models that never read it, so
        // kernel state = model state - 1 is all the wrapper amounts to; pmx_plan.cpp build_class_plan)
        int out_state = m.out[0].state - m.pm;
        double inv_vol = inv_vol0;
        if (oq != 0) {  // outputs beyond the first: rare, re-derive the volume instead of keeping 4 live
          // ONE descriptor fetch each for state and volume (the host resolved "theta index behind the volume", derived
          // values without covariate factors included: DevModel::out_vol_theta).  The compiler hoists these scalar
          // fetches in front of the branch, into every observation step of the single-output case: with the six
          // fetches + select chain of a device-side resolution C3 went from 0.83 to 0.97 ms.
          //
          // The volume's load must be CONSUMED inside this block on every path: when the division sat behind an
          // exec-masked skip (lanes with complex roots), the load was still pending at the join and the waitcnt pass
          // put `s_waitcnt vmcnt(0)` into the common emit path - every observation step then waited for all earlier
          // prediction stores (C3 0.83 -> 0.98 ms).  Hence: divide unconditionally, pin the quotient, select after.
          out_state = m.out[oq].state - m.pm;
          const int vp = m.out_vol_theta[oq];
          double v = 1.0;
          if (vp >= 0) v = th[vp];  // (scalar condition)
          double iv = 1.0 / v;
          asm volatile("" : "+v"(iv));
          inv_vol = ((lane_good || !LL) && !lane_badlag) ? iv : __longlong_as_double(0x7ff8000000000000LL);
        }
        if constexpr (LL) {
          // fold the G predictions into the members' sums instead of storing them (ll_accumulate, per member;
          // the observed values and sigma terms are wave-uniform scalar fetches)
          // the step's 3 x G scalars are fetched unconditionally and up front (a few wide s_loads instead of 3 G
          // dependent ones behind the weight test: the kernel was scalar-fetch-latency bound)
          const auto ov = as_const(cp.cobs) + cobs_off;
          double ov_y[G], ov_w[G];
#pragma unroll
          for (int j = 0; j < G; ++j) {
            ov_y[j] = kUpfront ? up_y[j] : ov[j];
            ov_w[j] = kUpfront ? up_w[j] : ov[G + j];
          }
          // one member-observation: d = y_obs - pred ; sum -= w d^2   (the constants come in at the end: csum).  The
          // weight tests are on the BITS (scalar integer compares; a floating-point compare of two SGPR values is a
          // vector instruction); the output's state is picked by a scalar branch around the whole member loop
          auto fold = [&](auto st_c) {
            constexpr int ST = decltype(st_c)::value;
            if constexpr (!DYNC) {
              // the common step: a plain row for every live member - no tests (a scalar branch per member costs more
              // than the three instructions it guards); padding members carry weight 0 and finite states: they add -0
              if (kobs < 63 && ((plain_obs >> kobs) & 1ull)) {
#pragma unroll
                for (int j = 0; j < G; ++j) {
                  const double d = fma(-inv_vol, x[j][ST], ov_y[j]);
                  ll_acc[j] = fma(-(d * ov_w[j]), d, ll_acc[j]);
                }
                return;
              }
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
              const int64_t wb = __double_as_longlong(ov_w[j]);
              if (wb != 0) {  // wave-uniform; weight 0 = missing observation (or chunk padding)
                if (CENS && wb < 0) {  // censored row (marker from pmx_ll_prepare_chunks): the generic fold on its full record
                  double y = x[j][ST] * inv_vol;
                  if constexpr (DYNC) {
                    y = ((cplx >> j) & 1u) ? __longlong_as_double(0x7ff8000000000000LL)
                                           : lane_out<KID>(m, Ld, x[j], 0.0, oq, cp.faco + (voff + j) * cp.n_fac);
                  }
                  ll_accumulate(as_const(ops.ll_obs) + (chunk_row[c * G + j] + kobs) * 4, y, ll_acc[j]);
                } else {
                  double d;
                  if constexpr (DYNC) {
                    const double y = ((cplx >> j) & 1u) ? __longlong_as_double(0x7ff8000000000000LL)
                                                        : lane_out<KID>(m, Ld, x[j], 0.0, oq, cp.faco + (voff + j) * cp.n_fac);
                    d = ov_y[j] - y;
                  } else {
                    d = fma(-inv_vol, x[j][ST], ov_y[j]);
                  }
                  ll_acc[j] = fma(-(d * ov_w[j]), d, ll_acc[j]);
                }
              }
            }
          };
          if constexpr (DYNC) {
            fold(std::integral_constant<int, 0>{});  // (lane_out picks the state itself)
          } else {
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
          }
          cobs_off += 2 * G;
          ++kobs;
        } else {
          if constexpr (DYNC) {
            double ys[G][1];  // each member's prediction under its own volume (NaN while its occasion has complex roots)
#pragma unroll
            for (int j = 0; j < G; ++j)
              ys[j][0] = ((cplx >> j) & 1u) ? __longlong_as_double(0x7ff8000000000000LL)
                                            : lane_out<KID>(m, Ld, x[j], 0.0, oq, cp.faco + (voff + j) * cp.n_fac);
            classed_emit<0, G, 1>(ys, 1.0, slot, kld, upper, pair_full, pair_half, any_half, n_live, bad);
          } else {
            // wave-uniform: the state is picked by a scalar branch, not per-lane selects
            classed_emit_state<0, G, NS>(out_state, x, inv_vol, slot, kld, upper, pair_full, pair_half, any_half, n_live,
                                         bad);
          }
          kld += ld;
        }
      }
    }
    if constexpr (DYNC) {
      cplx |= cplx_any;
      bad |= bad_any;
    }
    if constexpr (LL) {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (j < n_live) {
          const int64_t sid = chunk_subj[c * G + j];
          const double llj = ll_acc[j] + as_const(cp.cobs)[as_const(cp.chunk_obs_off)[c] + j];  // + the member's constants
          if (!isfinite(llj)) bad |= (1u << j);  // NonFiniteLikelihood (prediction.rs:119-124)
          if (lane_ok) ops.ll_out[sid * ops.ll_ld + p] = llj;  // (NaN already for a lane with complex roots)
        }
      }
    }
    // status bytes: the library zeroes the array before the launch (PMX_PAIR_OK == 0); only failures are
    // written here, so the healthy case issues no byte stores at all
    if (status != nullptr && (cp.zero_status == 2 || __any(((bad != 0u || cplx != 0u || !lane_good || lane_badlag) && lane_ok) ? 1 : 0))) {
      if (cp.zero_status == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clearing store above lands first
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (j < n_live) {
          const int64_t sid = chunk_subj[c * G + j];
          const uint8_t st = (!lane_good || ((cplx >> j) & 1u)) ? PMX_PAIR_COMPLEX_ROOTS
                             : (lane_badlag ? PMX_PAIR_BAD_LAG : (((bad >> j) & 1u) ? PMX_PAIR_NONFINITE : PMX_PAIR_OK));
          if (lane_ok && (st != PMX_PAIR_OK || cp.zero_status == 2)) status[sid * P + p] = st;
        }
      }
    }
  }
}


}  // namespace

hipError_t launch_classed(const LaunchArgs& a, const Route& r) {
  return with_kid(a.m.kernel, [&](auto kid) {
    return dispatch([&](auto ll, auto cens, auto perdt, auto lag, auto dync) {
      constexpr bool LL = decltype(ll)::value, CENS = decltype(cens)::value, PERDT = decltype(perdt)::value,
                     LAG = decltype(lag)::value, DYNC = decltype(dync)::value;
      // (no censored prediction pass; loose chunks: no lag classes; covariate rebuilds: loose chunks only)
      if constexpr ((CENS && !LL) || (LAG && PERDT) || (DYNC && !PERDT)) {
        return hipErrorInvalidValue;
      } else {
        hipLaunchKernelGGL((pmx_analytical_classed<decltype(kid)::value, LL, PERDT, LAG, CENS, DYNC>), dim3(static_cast<uint32_t>(r.blocks)),
                           dim3(r.threads), 0, static_cast<hipStream_t>(a.stream), a.m, a.ops, a.cls, a.theta, a.P, r.cpb, r.n_ptiles,
                           a.pred, a.ld, a.status);
        return hipGetLastError();
      }
    }, r.ll, r.ll && r.cens, r.loose, r.lag, r.dyn && !r.lag && r.loose);
  });
}

}  // namespace pmx

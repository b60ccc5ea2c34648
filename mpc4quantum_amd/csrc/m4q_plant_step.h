// m4q_plant_step.h - the step of the two descent methods on the plant itself: the Gauss-Newton SQP (m4q_plant_sqp_batch) and the iLQR
// (m4q_plant_ilqr_batch; mpc4quantum_amd/plant_sqp.py: _descent_reference is the definition of both).  Between two QPs on the
// plant's own linearisation (launch_plant_qp, unchanged) this kernel searches over `steps` candidates on the TRUE plant, takes the
// member's decision and hands the accepted trajectory to the next linearisation - the iterate never leaves the device.  ONE body
// (plant_step_kernel<PLANT, CLOSED>) for both methods.  What differs is the candidate, and that alone stands under `if constexpr
// (CLOSED)`: where the raw control w of step t comes from and how that step's operands (xb_t[j], ub_t, ...) are fetched.  The two
// forms are blocks of the one body and not a policy object handed to it: with an object (its source held by value or by reference,
// the flags as members or as arguments) the optimiser's output differed from the two earlier kernels' in every variant tried, and
// the one that was built changed all thirty kernels and took the closed-loop kernel at (16, 3) from 356 + 100 registers to
// 358 + 102; the blocks compile to the earlier kernels' instructions.
//
// Included by m4q_kernels.hip inside its shape namespace, behind plant_qp_kernel: the kernel is written on that file's NX, NU,
// LaneGeo, QuadRow, quad_figure and M4Q_PLANT_STEP - the forward step is the device function plant_rollout_kernel calls, on operands
// formed as that kernel forms them (u_scale[b][k] u[t][k] in fp64, dts[t]), so a trajectory stored here has the bits of
// m4q_plant_rollout_batch under the returned controls.
//
// One DPP row per member, launch_aux's grid over quads of members.  A pass rolls one control sequence from x0 with the state in
// registers and sums J = sum_t (x_t - xb_t)^H Q_t (x_t - xb_t) + (u_t - ub_t)^T R_t (u_t - ub_t) + the terminal term.  Passes
// 0 .. steps-1 are the candidates clip(U + 2^-p D), D = U_opt - U (one fma: 2^-p D is exact), and store nothing; the last pass is
// the winner again - THE SAME loop body, stores enabled, so its states and its J have the candidate's bits - and writes the controls,
// the T linearisation points where plant_factor_kernel reads them ([B][T][n]: PlantTraj::X has no member stride) and the full
// trajectory [B][T + 1][n].  iter < 0 is the initial roll: no candidates, the last pass on clip(U0).
// A member whose status is not SQP_RUNNING keeps everything it has; a quad of such members is skipped.
//
// CLOSED: a candidate is not that point of the line but the QP's law run on the true plant around the iterate
// (Xbar, Ubar) = (X_lin, U), its feed-forward part scaled by the step length a = 2^-p:
//     free:    ff = Re(K_t (Xbar_t - xb_t)) + Re(k_t) + ub_t - Ubar_t,   fb = Re(K_t (x_t - Xbar_t))
//     pinned:  ff = U_qp[t] - Ubar_t,  fb = 0      (exact mode, U_qp[t][k] on a bound: the slot holds a multiplier row, not a policy)
//     u_t = clip(fma(a, ff, Ubar_t) + fb)
// x_0 = Xbar_0 bit for bit (both are x0), so fb = 0 at t = 0; at a = 1 a free control is the stored law of m4q_feedback.h on the
// true plant, as a -> 0 the candidate is the iterate.  Lane j holds Xbar_t[j] and its m gain entries K_t[j][k]; the affine entries,
// U_qp[t] and Ubar_t are replicated over the row; the operands of step t + 1 are fetched while step t computes.
//
// The last pass overwrites U and X_lin IN PLACE while it reads them.  That is ordered: every address of the two arrays is read and
// written by one wavefront alone (a row past the end of the ensemble repeats the last member's reads and stores nothing); within
// it the loads of step t (issued during step t - 1, before the loop, or at the top of step t) come before the stores of step t in
// program order, through pointers the compiler may not assume distinct, and the vector memory pipeline keeps a wavefront's
// accesses to one address in issue order.  No later pass follows the storing one, so nothing reads what it wrote before the next
// launch on the stream.

constexpr int SQP_RUNNING = 0;        // (what a member that used up its iterations is left with: status 0)
constexpr int SQP_CONVERGED = 1, SQP_NO_DESCENT = 2, SQP_NOT_FINITE = 3;

struct IlqrOps {
  cplx xl, xb, Kx[NU];
  double kre[NU], uq[NU], uc[NU], ub[NU];
};
// Whether the replicated operands of step t + 1 are fetched ahead with the lane's own.  Not at n = 9: two wavefronts per SIMD leave
// 256 registers, which the full look-ahead overflows by 13 at m = 2 (56 bytes of scratch); fetched at the top of their own step
// they are 4 m doubles that every lane of the row reads from one address, behind the long plant step of the step before.
constexpr bool ROW_AHEAD = NX != 9;

template <int PLANT, bool CLOSED>
__global__ __launch_bounds__(64) M4Q_OCC void plant_step_kernel(PlantStepArgs a) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant has no linearisation kernel");
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * SCRATCH_ELEMS;
  const int T = a.T;
  const bool init = a.iter < 0;
  const bool exact = (a.flags & QP_EXACT_BOX) != 0;
  const int ncand = init ? 0 : a.steps;
  const int nquads = quads_of(a.B);
  const unsigned sX = (unsigned)(T + 1) * NX, sL = (unsigned)T * NX, sU = (unsigned)T * NU, sG = (unsigned)T * (NX + 1) * NU;
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const bool live = r.valid && (init || gld(a.status, r.b) == SQP_RUNNING);
    if (!__any(live)) continue;                      // (wave-uniform: every lane stays in step for the broadcasts below)
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const GView xbm = gview(a.X_bm, r.q0 * a.xbm_stride, r.gl * (unsigned)a.xbm_stride);
    const GView ubm = gview(a.U_bm, r.q0 * a.ubm_stride, r.gl * (unsigned)a.ubm_stride);
    const GView U0 = gview(a.U0, r.q0 * a.u0_stride, r.gl * (unsigned)a.u0_stride);
    const GView Uc = gview(a.U, r.q0 * sU, r.gl * sU);
    const GView Uq = gview(a.U_qp, r.q0 * sU, r.gl * sU);
    const GView Kg = gview(a.gains, r.q0 * sG, r.gl * sG);
    const GView Xl = gview(a.X_lin, r.q0 * sL, r.gl * sL);
    const GView Xo = gview(a.X, r.q0 * sX, r.gl * sX);
    // CLOSED: the operands of step t: the initial roll reads the first guess alone (no QP has run: X_lin, U_qp and the gains hold
    // nothing yet) ... in two parts: what a lane holds of its own (Xbar_t[j], xb_t[j], K_t[j][.]) and what is replicated over the row
    auto load_lane = [&](int t, IlqrOps& o) __attribute__((always_inline)) {
      o.xb = xbm.ld<cplx>(t * NX + j);
      o.xl = init ? o.xb : Xl.ld<cplx>(t * NX + j);
      const unsigned gt = (unsigned)t * (NX + 1) * NU;
#pragma unroll
      for (int k = 0; k < NU; ++k) o.Kx[k] = init ? czero() : Kg.ld<cplx>(gt + j * NU + k);
    };
    auto load_row = [&](int t, IlqrOps& o) __attribute__((always_inline)) {
      const unsigned gt = (unsigned)t * (NX + 1) * NU;
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        o.ub[k] = ubm.ld<double>(t * NU + k);
        o.uc[k] = init ? U0.ld<double>(t * NU + k) : Uc.ld<double>(t * NU + k);
        o.uq[k] = init ? 0.0 : Uq.ld<double>(t * NU + k);
        o.kre[k] = init ? 0.0 : Kg.ld<cplx>(gt + NX * NU + k).re;
      }
    };
    double sc[NU], lo0[NU], hi0[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      sc[k] = a.u_scale ? gld(a.u_scale, r.b * NU + k) : 1.0;
      const bool band = (a.flags & QP_DU_BAND) != 0 && a.u_prev != nullptr;
      const double up = band ? gld(a.u_prev, r.b * NU + k) : 0.0;
      lo0[k] = band ? fmax(-a.sat, up - a.du) : -a.sat;
      hi0[k] = band ? fmin(a.sat, up + a.du) : a.sat;
    }
    const cplx x0 = gld(a.x0, r.b * NX + j);
    const double Jcur = init ? 0.0 : gld(a.cost, r.b);
    double bestJ = 0.0, bestA = 1.0, Jp = 0.0;
    bool have = false, store = false;
    for (int p = 0; p <= ncand; ++p) {
      const bool last = p == ncand;
      if (last) {
        store = live && (init || (have && bestJ < Jcur));
        if (!__any(store)) break;
      }
      const double alpha = last ? bestA : __builtin_ldexp(1.0, -p);
      const bool stx = store && L.lane_ok, st0 = store && jj == 0;
      cplx x = x0;
      Jp = 0.0;
      IlqrOps nxt;                                   // (CLOSED alone: the operands fetched ahead, and below those of this step)
      if constexpr (CLOSED) {
        load_lane(0, nxt);
        if constexpr (ROW_AHEAD) load_row(0, nxt);
      }
      for (int t = 0; t < T; ++t) {
        IlqrOps cur;
        cplx dl, dx;
        if constexpr (CLOSED) {
          cur = nxt;
          if constexpr (!ROW_AHEAD) load_row(t, cur);
          const int tn = t + 1 < T ? t + 1 : t;
          load_lane(tn, nxt);
          if constexpr (ROW_AHEAD) load_row(tn, nxt);
          dl = csub(cur.xl, cur.xb), dx = csub(x, cur.xl);
        }
        double u[NU], v[NU], eu[NU];
#pragma unroll
        for (int k = 0; k < NU; ++k) {
          double w;                                  // the candidate's control before the clip
          if constexpr (!CLOSED) {                   // ... the point of the line, its operands loaded where they are used
            if (init) {
              w = U0.ld<double>(t * NU + k);
            } else {
              const double uc = Uc.ld<double>(t * NU + k);
              w = __builtin_fma(alpha, Uq.ld<double>(t * NU + k) - uc, uc);
            }
          }
          const double lo = t == 0 ? lo0[k] : -a.sat, hi = t == 0 ? hi0[k] : a.sat;
          if constexpr (CLOSED) {                    // ... the law around the iterate (the pin test reads the bounds)
            w = cur.uc[k];
            if (!init) {
              const double lin = rowsum<NX>(real_of(cmul(cur.Kx[k], dl))) + cur.kre[k] + cur.ub[k];
              const double loop = rowsum<NX>(real_of(cmul(cur.Kx[k], dx)));
              const bool pinned = exact && (cur.uq[k] >= hi || cur.uq[k] <= lo);
              const double ff = (pinned ? cur.uq[k] : lin) - cur.uc[k];
              const double fb = pinned ? 0.0 : loop;
              w = __builtin_fma(alpha, ff, cur.uc[k]) + fb;
            }
          }
          w = w < lo ? lo : w;                       // min(max(w, lo), hi) that lets a NaN through, as NumPy's does
          w = w > hi ? hi : w;
          u[k] = w;
          v[k] = sc[k] * w;
          eu[k] = w - (CLOSED ? cur.ub[k] : ubm.ld<double>(t * NU + k));
        }
        double cu = 0.0;
#pragma unroll
        for (int k = 0; k < NU; ++k)
#pragma unroll
          for (int l = 0; l < NU; ++l) cu += eu[k] * gld(a.R_ls, ((long)t * NU + k) * NU + l).re * eu[l];
        Jp += quad_figure<NX>(csub(x, CLOSED ? cur.xb : xbm.ld<cplx>(t * NX + j)), a.Q_ls + ((long)t * NX + j) * NX) + cu;
        if (st0) {
#pragma unroll
          for (int k = 0; k < NU; ++k) Uc.st<double>(t * NU + k, u[k]);
        }
        if (stx) {
          Xl.st<cplx>(t * NX + j, x);
          Xo.st<cplx>(t * NX + j, x);
        }
        M4Q_PLANT_STEP(PLANT, x, x, v, op0, ops, gld(a.dts, t), scratch, j, jj);
      }
      Jp += quad_figure<NX>(csub(x, xbm.ld<cplx>(T * NX + j)), a.Q_ls + ((long)T * NX + j) * NX);
      if (stx) Xo.st<cplx>(T * NX + j, x);
      // the smallest p attaining the minimum; a cost that is not finite is never chosen
      const bool better = !last && Jp - Jp == 0.0 && (!have || Jp < bestJ);
      bestJ = better ? Jp : bestJ;
      bestA = better ? alpha : bestA;
      have = have || better;
    }
    // the member's record.  (store: Jp is the cost of what the last pass stored.)
    const bool st0 = live && jj == 0;
    if (init) {
      if (st0) {
        gst(a.cost, r.b, Jp);
        gst(a.n_iter, r.b, 0);
        gst(a.status, r.b, Jp - Jp == 0.0 ? SQP_RUNNING : SQP_NOT_FINITE);
      }
      for (int e = jj; e <= a.iters; e += 16)
        if (live) gst(a.cost_hist, r.b * (a.iters + 1) + e, Jp);
      for (int e = jj; e < a.iters; e += 16)
        if (live) gst(a.alpha_hist, r.b * a.iters + e, 0.0);
    } else {
      if (st0 && !store) gst(a.status, r.b, SQP_NO_DESCENT);
      if (st0 && store) {
        gst(a.cost, r.b, Jp);
        gst(a.alpha_hist, r.b * a.iters + a.iter, bestA);
        gst(a.n_iter, r.b, a.iter + 1);
        if (Jcur - Jp <= a.tol * Jcur) gst(a.status, r.b, SQP_CONVERGED);
      }
      for (int e = a.iter + 1 + jj; e <= a.iters; e += 16)
        if (store) gst(a.cost_hist, r.b * (a.iters + 1) + e, Jp);
    }
    wave_sync();                                     // the rows' reads of their LDS blocks are done
  }
}

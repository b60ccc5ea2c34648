// m4q_feedback.h - a stored feedback law applied inside a rollout (FeedbackArgs, m4q_args.h; feedback.py is the definition):
//     u_t[k] = clip(sum_j Re(K_t[j][k] (x_t - xbar_t)_j) + Re(K_t[n][k]) + ubar_t[k])
// the expression of rollout_forward (m4q_mpc.h, lqr.py:74-76) on gains [N][n + 1][m] as quad_program_batch returns them, with the
// band p +- du around the control applied before at EVERY step, not only at the first.
// Included by m4q_kernels.hip after m4q_mpc.h (cplx, gld, rowsum).
#pragma once
#include "m4q_args.h"

namespace m4q {

// One member's law on its DPP row: lane j holds d_j = x_j - xbar_t[j] and K_t[j][0..NU); lanes >= NX shadow lane NX - 1 and are
// not among the NX lanes rowsum<NX> adds.  The operands of step t + 1 are fetched while step t computes, as RollCtl fetches the
// controls of an open-loop rollout.  Everything but xb and Kx is replicated over the row; t and the band are wave-uniform.
template <int NX, int NU>
struct FeedbackRow {
  const M4Q_GLOBAL cplx* K;        // the member's (or the shared) gains [N][NX + 1][NU]
  const M4Q_GLOBAL cplx* xr;       // ... x_ref [N][NX]
  const M4Q_GLOBAL double* ur;     // ... u_ref [N][NU]
  int N, j;
  bool band;
  double sat, du;
  double sc[NU];                   // u_scale[b]
  double p[NU];                    // the control applied before
  int clipped;                     // (t, k) with a bound active so far
  bool bad;                        // a control was not finite
  // the operands of the next step
  cplx xb, Kx[NU];
  double kre[NU], ub[NU];

  __device__ __forceinline__ void fetch(int t) {
    xb = gld(xr, (long)t * NX + j);
    const long gt = (long)t * (NX + 1) * NU;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      Kx[k] = gld(K, gt + j * NU + k);
      kre[k] = gld(K, gt + NX * NU + k).re;
      ub[k] = gld(ur, (long)t * NU + k);
    }
  }
  __device__ __forceinline__ FeedbackRow(const FeedbackArgs& a, long b, int j_)
      : K(a.gains + b * a.law_per * ((long)a.roll.N * (NX + 1) * NU)), xr(a.x_ref + b * a.law_per * ((long)a.roll.N * NX)),
        ur(a.u_ref + b * a.law_per * ((long)a.roll.N * NU)), N(a.roll.N), j(j_), band(a.du_band != 0), sat(a.sat), du(a.du), clipped(0),
        bad(false) {
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      sc[k] = a.roll.u_scale ? gld(a.roll.u_scale, b * NU + k) : 1.0;
      p[k] = band ? gld(a.u_prev, b * a.u_prev_stride + k) : 0.0;
    }
    fetch(0);
  }
  // step t in state x (this lane's entry): u = the commanded controls, v = u_scale[b] u what the plant sees
  __device__ __forceinline__ void take(int t, cplx x, double (&u)[NU], double (&v)[NU]) {
    const cplx dx = csub(x, xb);
    double part[NU], k0[NU], u0[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      part[k] = real_of(cmul(Kx[k], dx));
      k0[k] = kre[k];
      u0[k] = ub[k];
    }
    fetch(t + 1 < N ? t + 1 : t);
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      const double s = rowsum<NX>(part[k]) + k0[k] + u0[k];
      double lo = -sat, hi = sat;
      if (band) {
        lo = fmax(lo, p[k] - du);
        hi = fmin(hi, p[k] + du);
      }
      const double uk = fmin(fmax(s, lo), hi);
      clipped += (s <= lo || s >= hi) ? 1 : 0;
      bad = bad || !finite_d(uk);
      u[k] = p[k] = uk;
      v[k] = sc[k] * uk;
    }
  }
};

}  // namespace m4q

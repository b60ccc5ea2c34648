// m4q_plant_param.h - device functions of the plant-parameter gradient (m4q_plant_rollout_param_grad_batch): the adjoint step of
// the two unitary plants in the directions of a drift perturbation.  mpc4quantum_amd/plant_param.py (plant_param_grad_reference) is
// the definition; what is here follows it.
//
// The member's drift is op0_b + sum_j theta_j D_j, evaluated at the op0_b passed in.  A derivative in the direction D_j is the
// control gradient's construction (m4q_grad.h) with E_j = -i dt D_j in place of -i dt H_k: ONE matrix exponential of the
// (1 + PT) d block matrix
//     Z = [[X, E_1, .., E_PT], [0, X, 0, ..], .., [0, .., 0, X]],   X = -i dt (H0 + sum_k v_k H_k)
// holds U in block (0, 0) and dU_e = L(X, E_e) in block (0, 1 + e).  The PT directions are the p matrices of `dirs` and, when the
// drive gains are asked for too, the m control operators with E = -i dt u[t][k] H_k (dX/du_scale_k: the member sees
// v_k = u_scale_k u[t][k]).  PT is a template parameter, (1 + PT) d <= 16: lane c of the row owns column c of Z and expm_cols
// applies as it stands.  plant_grad_step (m4q_grad.h) is left as it is - this is its sibling over PT directions.
#pragma once
#include "m4q_grad.h"

namespace m4q {

// LDS of one row in the backward pass: F = [U, dU_1 .. dU_PT] ((1 + PT) d^2), then x_t, lam, P, Q, T (n each)
template <int NX, int PT, int D>
constexpr int param_scratch_elems() { return (1 + PT) * D * D + 5 * NX; }

// [U, dU_1 .. dU_PT] of one held-control step into F (LDS, [1 + PT][D][D] row-major): lane jj < (1 + PT) D owns column jj of Z.
// Direction e < p is dirs[e]; direction e >= p is control operator e - p scaled by the unscaled control ut[e - p].
// Every index into Dk and Hk is clamped into its array: a lane that owns no such block reads a valid entry and drops it.
template <int NU, int PT, int D>
__device__ __forceinline__ void param_block_expm(cplx* F, const double (&v)[NU], const double (&ut)[NU], int p, const GView& H0,
                                                 const GView& Hk, const GView& Dk, double dt, int jj) {
  constexpr int M = (1 + PT) * D;
  static_assert(M <= 16, "the block matrix of a step must fit the 16 lanes of a row");
  const int jb = jj < M ? jj : M - 1;
  const int kb = jb / D, cc = jb - kb * D;                 // block column and the column inside it
  const int e = kb > 0 ? kb - 1 : 0;                       // the direction this lane's column holds (kb > 0)
  const bool is_dir = e < p;
  const int kd = is_dir ? e : p - 1;                       // (1 <= p <= PT: both clamps stay inside dirs [p] and ops [NU])
  int kh = e - p;
  kh = kh < 0 ? 0 : (kh > NU - 1 ? NU - 1 : kh);
  double fac = 1.0;
#pragma unroll
  for (int k = 0; k < NU; ++k) fac = (!is_dir && kh == k) ? ut[k] : fac;
  const double sdt = dt * fac;
  cplx X[D], E[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    cplx hsum = H0.ld<cplx>(i * D + cc);
#pragma unroll
    for (int k = 0; k < NU; ++k) cmac_r(hsum, Hk.ld<cplx>((k * D + i) * D + cc), v[k]);
    X[i] = mk(hsum.im * dt, -hsum.re * dt);                // -i dt H
    const cplx dk = Dk.ld<cplx>((kd * D + i) * D + cc);
    const cplx hk = Hk.ld<cplx>((kh * D + i) * D + cc);
    const cplx dm = csel(is_dir, dk, hk);
    E[i] = mk(dm.im * sdt, -dm.re * sdt);                  // -i dt D_e, or -i dt u_k H_k
  }
  cplx Z[M];
#pragma unroll
  for (int r = 0; r < M; ++r) {
    const int rb = r / D, ri = r - rb * D;
    const cplx off = (rb == 0) ? csel(kb > 0, E[ri], czero()) : czero();
    Z[r] = csel(kb == rb, X[ri], off);
  }
  expm_cols<M>(Z, jb);
  if (jj < M) {
#pragma unroll
    for (int a = 0; a < D; ++a) F[(kb * D + a) * D + cc] = Z[a];
  }
}

// One backward step of the Hamiltonian (NC = 1, n = D^2) or process (NC = D^2, n = D^4: the same on every column c of the
// d^2 x d^2 matrix) plant, as plant_grad_step, over the PT directions of param_block_expm.  Lane j holds entry ((a D + e) NC + c)
// of x_t (x) and of lam_{t+1} (lam).
//   ge[k] = Re(lam^H vec_r(dU_k rho U^H + U rho dU_k^H)),   returns lam_t = vec_r(U^H Lam U)
// sc: the row's param_scratch_elems() of LDS.  One wave per block: wave_sync() is the wave's own LDS fence.
template <int NX, int NU, int PT, int D, int NC>
__device__ __forceinline__ cplx param_grad_step(cplx x, cplx lam, const double (&v)[NU], const double (&ut)[NU], int p, const GView& H0,
                                                const GView& Hk, const GView& Dk, double dt, cplx* sc, int j, int jj, double (&ge)[PT]) {
  static_assert(D * D * NC == NX, "state is a vectorised d x d matrix, or d^2 columns of them");
  cplx* F = sc;                          // [1 + PT][D][D]
  cplx* Rs = F + (1 + PT) * D * D;       // x_t
  cplx* Ls = Rs + NX;                    // lam_{t+1}
  cplx* Ps = Ls + NX;                    // rho U^H
  cplx* Qs = Ps + NX;                    // U rho
  cplx* Ts = Qs + NX;                    // U^H Lam
  param_block_expm<NU, PT, D>(F, v, ut, p, H0, Hk, Dk, dt, jj);
  if (jj < NX) { Rs[jj] = x; Ls[jj] = lam; }
  wave_sync();
  const int r = j / NC, c = j - r * NC;
  const int a = r / D, e = r - a * D;
  cplx pp = czero(), q = czero(), tt = czero();
#pragma unroll
  for (int g = 0; g < D; ++g) {
    cmac_cj(pp, F[e * D + g], Rs[(a * D + g) * NC + c]);         // sum_g rho[a][g] conj(U[e][g])
    cmac(q, F[a * D + g], Rs[(g * D + e) * NC + c]);             // sum_g U[a][g] rho[g][e]
    cmac_cj(tt, F[g * D + a], Ls[(g * D + e) * NC + c]);         // sum_g conj(U[g][a]) Lam[g][e]
  }
  if (jj < NX) { Ps[jj] = pp; Qs[jj] = q; Ts[jj] = tt; }
  wave_sync();
#pragma unroll
  for (int k = 0; k < PT; ++k) {
    const cplx* dU = F + (1 + k) * D * D;
    cplx y = czero();
#pragma unroll
    for (int g = 0; g < D; ++g) {
      cmac(y, dU[a * D + g], Ps[(g * D + e) * NC + c]);          // (dU_k rho U^H)[a][e]
      cmac_cj(y, dU[e * D + g], Qs[(a * D + g) * NC + c]);       // (U rho dU_k^H)[a][e]
    }
    ge[k] = rowsum<NX>(dot_re(lam, y));
  }
  cplx out = czero();
#pragma unroll
  for (int g = 0; g < D; ++g) cmac(out, Ts[(a * D + g) * NC + c], F[g * D + e]);       // sum_g (U^H Lam)[a][g] U[g][e]
  wave_sync();
  return out;
}

}  // namespace m4q

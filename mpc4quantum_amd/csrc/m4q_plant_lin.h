// m4q_plant_lin.h - device functions of the plant's own linearisation (m4q_plant_linearize_batch): the exact discrete-time
// Jacobians of one held-control step of the two unitary plants.  mpc4quantum_amd/plant_linearize.py (plant_linearize_reference) is
// the definition; what is here follows it.
//
// One 16-lane DPP row per (member, point) pair.  U and its Frechet derivatives dU_k come from the gradient's one matrix
// exponential of the (1 + m) d block matrix (m4q_grad.h: grad_block_expm); lane j of the row then owns entry j = (a, e, c) of the
// state x = vec_r(rho) (Hamiltonian plant, NC = 1) or of the process vector (NC = d^2 columns), as in plant_grad_step:
//     B[j][k]  = u_scale[k] (dU_k R U^H + U R dU_k^H)[a][e][c],   Delta_j = -sum_k B[j][k] u_k  (k ascending),
//     A[i][j'] = U[a][g] conj(U[e][h]) delta(c, c'),   i = (a, e, c), j' = (g, h, c'):  A does not depend on the state.
// The generator plant has no such kernel, for the reason m4q_grad.h gives.
#pragma once
#include "m4q_grad.h"

namespace m4q {

// LDS of one row: F = [U, dU_1 .. dU_m] ((1 + m) d^2), then x, P = R U^H, Q = U R (n each)
template <int NX, int NU, int D>
constexpr int plant_lin_scratch_elems() { return (1 + NU) * D * D + 3 * NX; }

// B[j][0 .. m) and Delta_j of one point for lane j, and F = [U, dU_k] left in sc for plant_lin_entry.
//   x: this lane's entry of the state; u: the controls as the caller passed them; s: the member's u_scale (the member sees s_k u_k)
// sc: the row's plant_lin_scratch_elems() of LDS.  One wave per block: wave_sync() is the wave's own LDS fence.  The caller fences
// once more before the next point overwrites sc.
template <int NX, int NU, int D, int NC>
__device__ __forceinline__ void plant_lin_point(cplx x, const double (&u)[NU], const double (&s)[NU], const GView& H0, const GView& Hk,
                                                double dt, cplx* sc, int j, int jj, cplx (&Bj)[NU], cplx& dlt) {
  static_assert(D * D * NC == NX, "state is a vectorised d x d matrix, or d^2 columns of them");
  cplx* F = sc;                          // [1 + NU][D][D]
  cplx* Rs = F + (1 + NU) * D * D;       // x
  cplx* Ps = Rs + NX;                    // rho U^H
  cplx* Qs = Ps + NX;                    // U rho
  double v[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) v[k] = s[k] * u[k];
  grad_block_expm<NU, D>(F, v, H0, Hk, dt, jj);
  if (jj < NX) Rs[jj] = x;
  wave_sync();
  const int r = j / NC, c = j - r * NC;
  const int a = r / D, e = r - a * D;
  cplx p = czero(), q = czero();
#pragma unroll
  for (int g = 0; g < D; ++g) {
    cmac_cj(p, F[e * D + g], Rs[(a * D + g) * NC + c]);          // sum_g rho[a][g] conj(U[e][g])
    cmac(q, F[a * D + g], Rs[(g * D + e) * NC + c]);             // sum_g U[a][g] rho[g][e]
  }
  if (jj < NX) { Ps[jj] = p; Qs[jj] = q; }
  wave_sync();
  dlt = czero();
#pragma unroll
  for (int k = 0; k < NU; ++k) {
    const cplx* dU = F + (1 + k) * D * D;
    cplx y = czero();
#pragma unroll
    for (int g = 0; g < D; ++g) {
      cmac(y, dU[a * D + g], Ps[(g * D + e) * NC + c]);          // (dU_k rho U^H)[a][e]
      cmac_cj(y, dU[e * D + g], Qs[(a * D + g) * NC + c]);       // (U rho dU_k^H)[a][e]
    }
    Bj[k] = cscale(y, s[k]);
    cmac_r(dlt, Bj[k], -u[k]);
  }
}

// A[i][col] from the U that plant_lin_point left in F: i = (a, e, c), col = (g, h, c')
template <int D, int NC>
__device__ __forceinline__ cplx plant_lin_entry(const cplx* F, int i, int col) {
  const int ri = i / NC, ci = i - ri * NC;
  const int rc = col / NC, cc = col - rc * NC;
  const int a = ri / D, e = ri - a * D;
  const int g = rc / D, h = rc - g * D;
  const cplx ug = F[a * D + g], uh = F[e * D + h];
  return csel(ci == cc, cmul(ug, cconj(uh)), czero());
}

}  // namespace m4q

// m4q_grad.h - device functions of the rollout gradients (m4q_plant_rollout_grad_batch, m4q_model_rollout_grad_batch):
// the adjoint step of the two unitary plants and the ordered ensemble reduction.  mpc4quantum_amd/grad.py
// (plant_rollout_grad_reference, model_rollout_grad_reference, ordered_weighted_sum) is the definition; what is here follows it.
//
// One 16-lane DPP row per member, as in the rollouts: lane j of a row owns entry j of the state x = vec_r(rho) and of the
// costate lam.  The forward pass is the rollouts' own step and leaves x_0 .. x_N in a device workspace; the backward pass reads x_t
// back, recomputes U and its Frechet derivatives dU_k from ONE matrix exponential of the (1 + m) d block matrix
//     Z = [[X, E_1, .., E_m], [0, X, 0, ..], .., [0, .., 0, X]],   X = -i dt (H0 + sum_k v_k H_k),  E_k = -i dt H_k:
// expm(Z) holds U in block (0, 0) and dU_k = L(X, E_k) in block (0, k).  Every compiled plant shape keeps (1 + m) d <= 16, the
// lanes of a row, so expm_cols<(1 + m) d> applies as it stands: lane c of the row owns column c of Z.
// The GENERATOR plant has no such kernel - its block matrix has (1 + m) n > 16 columns for n >= 9: dissipative dynamics go through
// the gradient of the discretised model (model_rollout_grad_kernel).
#pragma once
#include "m4q_args.h"
#include "m4q_mpc.h"

namespace m4q {

// LDS of one row in the backward pass of the plant gradient: F = [U, dU_1 .. dU_m] ((1 + m) d^2), then x_t, lam, P, Q, T (n each)
template <int NX, int NU, int D>
constexpr int grad_scratch_elems() { return (1 + NU) * D * D + 5 * NX; }

// g = (W + W^H) d for a row: entry j, with d distributed over the lanes.  W [N][N] row-major, shared by the ensemble
template <int N>
__device__ __forceinline__ cplx figure_grad(cplx d, const M4Q_GLOBAL cplx* W, int j) {
  cplx y = czero();
  static_for<0, N>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    const cplx dk = bcast<k>(d);
    cmac(y, gld(W, j * N + k), dk);           // W[j][k] d_k
    cmac_cj(y, gld(W, k * N + j), dk);        // conj(W[k][j]) d_k
  });
  return y;
}

// [U, dU_1 .. dU_m] of one held-control step into F (LDS, [1 + NU][D][D] row-major): lane jj < (1 + NU) D owns column jj of Z
template <int NU, int D>
__device__ __forceinline__ void grad_block_expm(cplx* F, const double (&v)[NU], const GView& H0, const GView& Hk, double dt, int jj) {
  constexpr int M = (1 + NU) * D;
  static_assert(M <= 16, "the block matrix of a step must fit the 16 lanes of a row");
  const int jb = jj < M ? jj : M - 1;
  const int kb = jb / D, cc = jb - kb * D;                 // block column and the column inside it
  const int ke = kb > 0 ? kb - 1 : 0;                      // the control whose E_k this lane's column holds (kb > 0)
  cplx X[D], E[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    cplx hsum = H0.ld<cplx>(i * D + cc);
#pragma unroll
    for (int k = 0; k < NU; ++k) cmac_r(hsum, Hk.ld<cplx>((k * D + i) * D + cc), v[k]);
    X[i] = mk(hsum.im * dt, -hsum.re * dt);                // -i dt H
    const cplx hk = Hk.ld<cplx>((ke * D + i) * D + cc);
    E[i] = mk(hk.im * dt, -hk.re * dt);                    // -i dt H_k
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
// d^2 x d^2 matrix) plant.  Lane j holds entry ((a D + e) NC + c) of x_t (x) and of lam_{t+1} (lam).
//   ge[k] = Re(lam^H vec_r(dU_k rho U^H + U rho dU_k^H)),   returns lam_t = vec_r(U^H Lam U)
// sc: the row's grad_scratch_elems() of LDS.  One wave per block: wave_sync() is the wave's own LDS fence.
template <int NX, int NU, int D, int NC>
__device__ __forceinline__ cplx plant_grad_step(cplx x, cplx lam, const double (&v)[NU], const GView& H0, const GView& Hk, double dt,
                                                cplx* sc, int j, int jj, double (&ge)[NU]) {
  static_assert(D * D * NC == NX, "state is a vectorised d x d matrix, or d^2 columns of them");
  cplx* F = sc;                          // [1 + NU][D][D]
  cplx* Rs = F + (1 + NU) * D * D;       // x_t
  cplx* Ls = Rs + NX;                    // lam_{t+1}
  cplx* Ps = Ls + NX;                    // rho U^H
  cplx* Qs = Ps + NX;                    // U rho
  cplx* Ts = Qs + NX;                    // U^H Lam
  grad_block_expm<NU, D>(F, v, H0, Hk, dt, jj);
  if (jj < NX) { Rs[jj] = x; Ls[jj] = lam; }
  wave_sync();
  const int r = j / NC, c = j - r * NC;
  const int a = r / D, e = r - a * D;
  cplx p = czero(), q = czero(), tt = czero();
#pragma unroll
  for (int g = 0; g < D; ++g) {
    cmac_cj(p, F[e * D + g], Rs[(a * D + g) * NC + c]);          // sum_g rho[a][g] conj(U[e][g])
    cmac(q, F[a * D + g], Rs[(g * D + e) * NC + c]);             // sum_g U[a][g] rho[g][e]
    cmac_cj(tt, F[g * D + a], Ls[(g * D + e) * NC + c]);         // sum_g conj(U[g][a]) Lam[g][e]
  }
  if (jj < NX) { Ps[jj] = p; Qs[jj] = q; Ts[jj] = tt; }
  wave_sync();
#pragma unroll
  for (int k = 0; k < NU; ++k) {
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

// The ordered ensemble reduction (grad.py: ordered_weighted_sum).  Thread (c, e) adds the rows of chunk c at element e in ascending
// order from 0.0; with weights every product is rounded before it is added (the empty asm keeps the compiler from contracting the
// two into an FMA).  Element e < nm comes from vals[i][e]; element nm is the row's objective: the sum of its q_cols figures, t
// ascending (q_cols > 0), or vals[i][nm] (q_cols == 0: a row of partial sums).  (GradReduceArgs: m4q_args.h)
__device__ __forceinline__ void grad_reduce(const GradReduceArgs& a) {
  const long E = (long)a.nm + 1;
  const long nchunks = ((long)a.count + a.chunk - 1) / a.chunk;
  const long total = nchunks * E;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
    const long c = id / E;
    const int e = (int)(id - c * E);
    const long i0 = c * a.chunk;
    const long i1 = i0 + a.chunk < a.count ? i0 + a.chunk : a.count;
    double acc = 0.0;
    for (long i = i0; i < i1; ++i) {
      double val;
      if (e < a.nm || a.q_cols == 0) {
        val = gld(a.vals, i * a.row_stride + e);
      } else {
        val = 0.0;
        for (int t = 0; t < a.q_cols; ++t) val = val + gld(a.q, i * a.q_cols + t);
      }
      if (a.w) {
        double prod = gld(a.w, i) * val;
        asm volatile("" : "+v"(prod));
        val = prod;
      }
      acc = acc + val;
    }
    if (e < a.nm) gst(a.out, c * a.out_stride + e, acc);
    else gst(a.out_last, c * a.last_stride, acc);
  }
}

}  // namespace m4q

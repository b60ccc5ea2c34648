// m4q_fit_qr.h - device functions of dmdc_fit_qr_kernel (m4q_kernels.hip): the batched DMDc fit A = Y pinv(Z, rcond) of
// m4q_dmdc_fit_qr_batch, taken from a QR of the data themselves and not from their Gram matrix, so that the error is
// O(eps kappa) and not O(eps kappa^2).  mpc4quantum_amd/fit.py (dmdc_fit_qr_reference) is the definition; what is here follows it
// operation by operation, so the two differ only by the device's sqrt and division and the compiler's FMA contraction.
//
// The frame and the LDS layout are dmdc_fit_kernel's (m4q_fit.h: FitLayout): one wavefront owns one member, R (then M) takes G's
// place, V its own, T takes C's (T[j][i] at C[i][j]).  Every snapshot contributes the row (z^H | y^H): Z^H = Q R, T = Q^H Y^H,
// then R V = M with orthogonal columns gives A = sum_k (T^H m_k / lam_k) v_k^H, the truncated product of m4q_fit.h.
//   Givens phase   lane l owns column l of R and of the incoming row (a register), lanes 0..n-1 also column l of T and of the
//                  right-hand side.  Rotation j takes c, s from R[j][j] and row[j], both read out of lane j (readlane: j is a
//                  loop counter); no lane reads LDS that another wrote, so the nz dependent rotations of a snapshot run
//                  without a wave_sync().
//   Hestenes phase lane l owns row l of M and of V, so a rotation of columns p, q touches the lane's own row only; the three
//                  inner products of the pair are sums over lanes: the 16 lanes of each DPP row in ascending order (rowsum),
//                  then the row sums in ascending order - fit.lane_sum.  The sums are wave-uniform, the skip is a scalar branch.
// All control flow is wave-uniform.
#pragma once
#include "m4q_fit.h"

namespace m4q {

// lane k's value in every lane (k uniform)
__device__ __forceinline__ double lane_value(double x, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k), __builtin_amdgcn_readlane(__double2loint(x), k));
}
__device__ __forceinline__ cplx lane_value(cplx x, int k) { return mk(lane_value(x.re, k), lane_value(x.im, k)); }

// The sum of v over the lanes 0..NZ-1 (the others hold 0), uniform: fit.lane_sum.
template <int NZ>
__device__ __forceinline__ double lane_sum(double v) {
  const double r = rowsum<(NZ < 16 ? NZ : 16)>(v);
  double s = lane_value(r, 0);
  if constexpr (NZ > 16) s += lane_value(r, 16);
  if constexpr (NZ > 32) s += lane_value(r, 32);
  if constexpr (NZ > 48) s += lane_value(r, 48);
  return s;
}

// (a', b') = (conj(c) a + conj(s) b, c b - s a): the Givens rotation [[conj(c), conj(s)], [-s, c]] on the rows a over b
__device__ __forceinline__ void givens_pair(cplx c, cplx s, cplx a, cplx b, cplx& an, cplx& bn) {
  an = mk((c.re * a.re + c.im * a.im) + (s.re * b.re + s.im * b.im), (c.re * a.im - c.im * a.re) + (s.re * b.im - s.im * b.re));
  bn = mk((c.re * b.re - c.im * b.im) - (s.re * a.re - s.im * a.im), (c.re * b.im + c.im * b.re) - (s.re * a.im + s.im * a.re));
}

// Phase 1: the streaming QR.  R = 0, T = 0; every snapshot's row (z^H | y^H) is rotated into them, j = 0 .. nz - 1.
// Returns false if R or T holds a non-finite entry (any non-finite sample produces one).
// REFIT (m4q_fit.h): only t < steps of every experiment; R <- discount R, T <- discount T before a snapshot's rotations, every lane
// on the entries it rotates; afterwards T[j][i] <- T[j][i] - sum_{k >= j} R[j][k] conj(A0[i][k]), k ascending, lane j on row j of R
// and of T.  Returns false for a non-finite A0, too.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ bool fit_qr_factor(const FitArgs& a, long b, cplx* lds, int lane, const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  cplx* R = lds + L::G;
  cplx* T = lds + L::C;
  const cplx* XN = lds + L::XN;
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  const bool rhs_lane = lane < NX;
  const int lt = rhs_lane ? lane : NX - 1;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i) R[i * PITCH + l] = czero();
#pragma unroll
    for (int i = 0; i < NX; ++i) T[i * PITCH + l] = czero();
  }
  [[maybe_unused]] int t = 0;
  fit_stream<NX, NU, ORDER>(a, b, lds, lane, [&](cplx z) {
    if constexpr (REFIT) {
      const bool taken = uniform(t < pr.steps);
      if (++t == a.N) t = 0;
      if (!taken) return;
      if (act) {
#pragma unroll 1
        for (int i = 0; i < NZ; ++i)
          if (i <= l) R[i * PITCH + l] = cscale(R[i * PITCH + l], pr.discount);
      }
      if (rhs_lane) {
#pragma unroll 1
        for (int j = 0; j < NZ; ++j) T[lt * PITCH + j] = cscale(T[lt * PITCH + j], pr.discount);
      }
    }
    cplx row = cconj(z);
    cplx rhs = cconj(XN[lt]);
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) {
      const cplx bj = lane_value(row, j);
      if (uniform(bj.re == 0.0 && bj.im == 0.0)) continue;
      const cplx rj = R[j * PITCH + l];
      const cplx tj = T[lt * PITCH + j];
      const cplx aj = lane_value(rj, j);
      const double h = sqrt((aj.re * aj.re + aj.im * aj.im) + (bj.re * bj.re + bj.im * bj.im));
      const cplx c = mk(aj.re / h, aj.im / h), s = mk(bj.re / h, bj.im / h);
      cplx rn, tn, rown, rhsn;
      givens_pair(c, s, rj, row, rn, rown);
      givens_pair(c, s, tj, rhs, tn, rhsn);
      if (act && l >= j) {
        R[j * PITCH + l] = rn;
        row = rown;
      }
      if (rhs_lane) {
        T[lt * PITCH + j] = tn;
        rhs = rhsn;
      }
    }
  });
  bool ok = true;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i)
      if (i <= l) ok = ok && finite_d(R[i * PITCH + l].re) && finite_d(R[i * PITCH + l].im);
#pragma unroll
    for (int i = 0; i < NX; ++i) ok = ok && finite_d(T[i * PITCH + l].re) && finite_d(T[i * PITCH + l].im);
  }
  wave_sync();
  if constexpr (REFIT) {
    const bool finite = !__any(!ok) && prior_finite<NX, NZ>(pr, l);
    if (uniform(finite)) {
      cplx d[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) d[i] = T[i * PITCH + l];
#pragma unroll 1
      for (int k = 0; k < NZ; ++k) {
        if (k >= l) {
          const cplx r = R[l * PITCH + k];
#pragma unroll
          for (int i = 0; i < NX; ++i) cmsub(d[i], r, cconj(gld(pr.A0, i * NZ + k)));
        }
      }
      if (act) {
#pragma unroll
        for (int i = 0; i < NX; ++i) T[i * PITCH + l] = d[i];
      }
      wave_sync();
    }
    return finite;
  }
  return !__any(!ok);
}

// Phase 2: one-sided (Hestenes) Jacobi on the columns of M = R, V = I accumulated: R V = M.  Pairs cyclic by rows; the rotation
// and the skip rule are fit_jacobi's, on a_pp = m_p^H m_p, a_qq = m_q^H m_q, g = m_p^H m_q.  Every lane reads and writes its
// own row of M and V only.  Returns true if a sweep skipped every pair within FIT_MAX_SWEEPS.
template <int NZ, int PITCH>
__device__ __forceinline__ bool fit_qr_jacobi(cplx* M, cplx* V, int lane) {
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i) V[l * PITCH + i] = mk(i == l ? 1.0 : 0.0, 0.0);
  }
#pragma unroll 1
  for (int sweep = 0; sweep < FIT_MAX_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll 1
    for (int p = 0; p < NZ - 1; ++p) {
#pragma unroll 1
      for (int q = p + 1; q < NZ; ++q) {
        const cplx mp = csel(act, M[l * PITCH + p], czero()), mq = csel(act, M[l * PITCH + q], czero());
        const double app = lane_sum<NZ>(mp.re * mp.re + mp.im * mp.im);
        const double aqq = lane_sum<NZ>(mq.re * mq.re + mq.im * mq.im);
        const cplx g = mk(lane_sum<NZ>(mp.re * mq.re + mp.im * mq.im), lane_sum<NZ>(mp.re * mq.im - mp.im * mq.re));
        const double m2 = g.re * g.re + g.im * g.im;
        if (uniform(m2 <= FIT_EPS * FIT_EPS * (app * aqq))) continue;
        rotated = true;
        const double absg = sqrt(m2);
        const double tau = (aqq - app) / (2.0 * absg);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t);
        const cplx sw = mk(t * c * (g.re / absg), t * c * (g.im / absg));
        cplx mpn, mqn, vp, vq;
        rotate_pair(c, sw, mp, mq, mpn, mqn);
        rotate_pair(c, sw, V[l * PITCH + p], V[l * PITCH + q], vp, vq);
        if (act) {
          M[l * PITCH + p] = mpn;
          M[l * PITCH + q] = mqn;
          V[l * PITCH + p] = vp;
          V[l * PITCH + q] = vq;
        }
      }
    }
    if (!rotated) return true;
  }
  return false;
}

// Phase 3: lam_k = m_k^H m_k, the singular values sqrt(lam) in descending order (by rank-counting in LDS, Z's place; this route
// needs no second pass over the data), W = T^H M divided by lam into T's place, then the truncated products of m4q_fit.h.
// ok = false: zero models, ranks and singular values.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ void fit_qr_models(const FitArgs& a, long b, cplx* lds, int lane, bool ok, const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  const cplx* M = lds + L::G;
  cplx* T = lds + L::C;
  double* LAM = reinterpret_cast<double*>(lds + L::LAM);
  double* S2 = reinterpret_cast<double*>(lds + L::Z);
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  double lam_l = 0.0, lmax = 0.0;
  wave_sync();
  if (uniform(ok)) {
#pragma unroll 1
    for (int k = 0; k < NZ; ++k) {
      const cplx m = csel(act, M[l * PITCH + k], czero());
      const double s = lane_sum<NZ>(m.re * m.re + m.im * m.im);
      lam_l = l == k ? s : lam_l;
      lmax = k == 0 ? s : fmax(lmax, s);
    }
  }
  if (act) {
    LAM[l] = lam_l;
    S2[l] = lam_l;
  }
  wave_sync();
  if (a.svals) {
    int pos = 0;
#pragma unroll 1
    for (int k = 0; k < NZ; ++k) {
      const double sk = S2[k];
      pos += (sk > lam_l || (sk == lam_l && k < l)) ? 1 : 0;
    }
    if (act) gst(a.svals, b * NZ + pos, sqrt(lam_l));
  }
  if (uniform(ok)) {
    cplx acc[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = czero();
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) {
      const cplx m = M[j * PITCH + l];
#pragma unroll
      for (int i = 0; i < NX; ++i) cmac_cj(acc[i], T[i * PITCH + j], m);       // += conj(T[j][i]) M[j][l]
    }
    wave_sync();
    const double inv = 1.0 / lam_l;
    if (act) {
#pragma unroll
      for (int i = 0; i < NX; ++i) T[i * PITCH + l] = cscale(acc[i], inv);
    }
  }
  wave_sync();
  fit_truncate<NX, NU, ORDER, REFIT>(a, b, lds, lane, ok, lmax, pr);
}

}  // namespace m4q

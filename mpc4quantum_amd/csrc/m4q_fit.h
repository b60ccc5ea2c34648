// m4q_fit.h - device functions of dmdc_fit_kernel (m4q_kernels.hip): the batched, truncated least-squares DMDc fit
// A = Y pinv(Z, rcond) of m4q_dmdc_fit_batch.  mpc4quantum_amd/fit.py (dmdc_fit_reference) is the definition; what is here follows
// it operation by operation, so the two differ only by the device's sqrt and division and the compiler's FMA contraction.
//
// ONE WAVEFRONT OWNS ONE MEMBER (nz = n (1 + P) runs to 64: a 16-lane DPP row cannot own a column).  Lane l owns index l of the
// nz axis: column l of G and C while the snapshots stream in, row l of G and V during a rotation, column l of A in the products.
// Everything between lanes goes through LDS: G [nz][PITCH], V [nz][PITCH], C [n][PITCH] complex, the current snapshot z [nz] and
// x_{t+1} [n], the eigenvalues [nz].  PITCH = nz | 1: an odd row pitch (in 16-byte elements) keeps both the accesses along a row
// (lane stride 16 B) and those down a column (lane stride PITCH 16 B) spread over the banks.
// All control flow is wave-uniform by construction (one member per wavefront); the rotation and truncation decisions are made
// uniform for the compiler too (readfirstlane), so they are scalar branches.
//
// REFIT (dmdc_refit_kernel, dmdc_refit_qr_kernel; RefitArgs): the fit against a prior model A0, A0 + (Y - A0 Z) pinv(Z, rcond) on
// the member's first `steps` snapshots of every experiment, weighted discount^(age) - fit.py's last part.  The flag adds to the
// functions below what FitPrior describes and leaves their REFIT = false instances as they were.
#pragma once
#include "m4q_args.h"
#include "m4q_mpc.h"

namespace m4q {

constexpr int FIT_MAX_SWEEPS = 30;                       // fit.MAX_SWEEPS
constexpr double FIT_EPS = 2.220446049250313e-16;        // np.finfo(np.float64).eps
constexpr size_t FIT_LDS_LIMIT = 160 * 1024;             // LDS of one gfx950 workgroup

template <int NX, int NU, int ORDER>
struct FitLayout {
  static constexpr int NZ = NX * (1 + PowTab<NU, ORDER>::NP);
  static constexpr int PITCH = NZ | 1;
  // offsets in cplx elements
  static constexpr int G = 0, V = G + NZ * PITCH, C = V + NZ * PITCH, Z = C + NX * PITCH, XN = Z + NZ, LAM = XN + NX;
  static constexpr int ELEMS = LAM + (NZ + 1) / 2;       // (the eigenvalues are doubles)
  static constexpr size_t BYTES = sizeof(cplx) * (size_t)ELEMS;
  static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;
};

__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

// The member's part of a fit against a prior model: its A0 [n][nz], the steps it takes of every experiment, its discount.
struct FitPrior {
  const M4Q_GLOBAL cplx* A0;
  int steps;
  double discount;
};

// acc -= a * b
__device__ __forceinline__ void cmsub(cplx& acc, cplx a, cplx b) {
  acc.re = fma(-a.re, b.re, acc.re);
  acc.re = fma(a.im, b.im, acc.re);
  acc.im = fma(-a.re, b.im, acc.im);
  acc.im = fma(-a.im, b.re, acc.im);
}

// Whether column l of the member's A0 is finite, for every lane: the prior's part of status 3.
template <int NX, int NZ>
__device__ __forceinline__ bool prior_finite(const FitPrior& pr, int l) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const cplx v = gld(pr.A0, i * NZ + l);
    ok = ok && finite_d(v.re) && finite_d(v.im);
  }
  return !__any(!ok);
}

// (a', b') = (c a - conj(sw) b, sw a + c b): columns p, q of M J for the rotation J = [[c, sw], [-conj(sw), c]]
__device__ __forceinline__ void rotate_pair(double c, cplx sw, cplx a, cplx b, cplx& an, cplx& bn) {
  an = mk(c * a.re - (sw.re * b.re + sw.im * b.im), c * a.im - (sw.re * b.im - sw.im * b.re));
  bn = mk((sw.re * a.re - sw.im * a.im) + c * b.re, (sw.re * a.im + sw.im * a.re) + c * b.im);
}

// The member's snapshots in their order, e outer, t inner: for each, z = [x_t ; lift(u_t) (x) x_t] goes to Z and x_{t+1} to XN in
// LDS, then body(z) runs with lane l holding z_l.  x_{t+1} (needed for XN now, for z next) and x_{t+2}, u_{t+1} are in flight
// while snapshot t is worked on.  Shared by the kernels that read training data (dmdc_fit_kernel, online_dmdc_kernel): L names
// where Z [NZ] and XN [NX] live in LDS, Args holds xs [B][E][N + 1][n], u, u_stride, u_scale, E and N.
template <int NX, int NU, int ORDER, class L = FitLayout<NX, NU, ORDER>, class Args = FitArgs, class F>
__device__ __forceinline__ void fit_stream(const Args& a, long b, cplx* lds, int lane, F body) {
  constexpr int NZ = L::NZ, NP = PowTab<NU, ORDER>::NP;
  cplx* Z = lds + L::Z;
  cplx* XN = lds + L::XN;
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  const int p = l / NX, jx = l - p * NX;
  double sc[NU];
#pragma unroll
  for (int k = 0; k < NU; ++k) sc[k] = a.u_scale ? gld(a.u_scale, b * NU + k) : 1.0;
  const int N = a.N;
  for (int e = 0; e < a.E; ++e) {
    const M4Q_GLOBAL cplx* xe = a.xs + ((b * a.E + e) * (long)(N + 1)) * NX;
    const M4Q_GLOBAL double* ue = a.u + b * a.u_stride + (long)e * N * NU;
    cplx xa = gld(xe, jx), xb = gld(xe, NX + jx);
    double un[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) un[k] = gld(ue, k);
    for (int t = 0; t < N; ++t) {
      const int t2 = t + 2 <= N ? t + 2 : N, t1 = t + 1 < N ? t + 1 : t;
      const cplx xc = gld(xe, (long)t2 * NX + jx);
      double ut[NU];
#pragma unroll
      for (int k = 0; k < NU; ++k) {
        ut[k] = sc[k] * un[k];
        un[k] = gld(ue, (long)t1 * NU + k);
      }
      Poly<NU, ORDER> poly;
      poly.eval(ut);
      double w = 1.0;
      static_for<0, NP>([&](auto pp) { w = p == decltype(pp)::value + 1 ? poly.pu[decltype(pp)::value] : w; });
      const cplx z = cscale(xa, w);
      wave_sync();                       // the reads of the previous snapshot are done
      if (act) Z[l] = z;
      if (lane < NX) XN[lane] = xb;
      wave_sync();
      body(z);
      xa = xb;
      xb = xc;
    }
  }
  wave_sync();
}

// Phase 1: G = sum z z^H (upper triangle accumulated, then mirrored), C = sum x_{t+1} z^H over the member's snapshots.
// The accumulators live in LDS: at nz = 64 they are 4096 + 1024 complex numbers, 160 doubles per lane, and the streaming phase is a
// small part of the run beside the rotations.  Returns false if G or C holds a non-finite entry.
// REFIT: only t < steps of every experiment; G <- d2 G, C <- d2 C before a snapshot is accumulated, d2 = discount^2 and the product
// rounded on its own; afterwards D = C - A0 G takes C's place, D[i][l] = C[i][l] - sum_k A0[i][k] G[k][l] with k ascending (lane l on
// column l; every lane reads the same A0[i][k]: a broadcast).  Returns false for a non-finite A0, too.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ bool fit_accumulate(const FitArgs& a, long b, cplx* lds, int lane, const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  cplx* G = lds + L::G;
  cplx* C = lds + L::C;
  const cplx* Z = lds + L::Z;
  const cplx* XN = lds + L::XN;
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i) G[i * PITCH + l] = czero();
#pragma unroll
    for (int i = 0; i < NX; ++i) C[i * PITCH + l] = czero();
  }
  [[maybe_unused]] const double d2 = pr.discount * pr.discount;
  [[maybe_unused]] int t = 0;
  fit_stream<NX, NU, ORDER>(a, b, lds, lane, [&](cplx z) {
    if constexpr (REFIT) {               // beyond the member's count the snapshot streams past
      const bool taken = uniform(t < pr.steps);
      if (++t == a.N) t = 0;
      if (!taken) return;
    }
    if (act) {
#pragma unroll 1
      for (int i = 0; i < NZ; ++i) {
        if (i <= l) {
          cplx g = G[i * PITCH + l];
          if constexpr (REFIT) g = cscale(g, d2);
          cmac_cj(g, z, Z[i]);           // += z_i conj(z_l)
          G[i * PITCH + l] = g;
        }
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        cplx c = C[i * PITCH + l];
        if constexpr (REFIT) c = cscale(c, d2);
        cmac_cj(c, z, XN[i]);
        C[i * PITCH + l] = c;
      }
    }
  });
  bool ok = true;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i) {
      if (i > l) G[i * PITCH + l] = cconj(G[l * PITCH + i]);
      else ok = ok && finite_d(G[i * PITCH + l].re) && finite_d(G[i * PITCH + l].im);
    }
    G[l * PITCH + l].im = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) ok = ok && finite_d(C[i * PITCH + l].re) && finite_d(C[i * PITCH + l].im);
  }
  wave_sync();
  if constexpr (REFIT) {
    const bool finite = !__any(!ok) && prior_finite<NX, NZ>(pr, l);
    if (uniform(finite)) {
      cplx d[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) d[i] = C[i * PITCH + l];
#pragma unroll 1
      for (int k = 0; k < NZ; ++k) {
        const cplx g = G[k * PITCH + l];
#pragma unroll
        for (int i = 0; i < NX; ++i) cmsub(d[i], gld(pr.A0, i * NZ + k), g);
      }
      if (act) {
#pragma unroll
        for (int i = 0; i < NX; ++i) C[i * PITCH + l] = d[i];
      }
      wave_sync();
    }
    return finite;
  }
  return !__any(!ok);
}

// Phase 2: G = V diag(lam) V^H by cyclic-by-rows Jacobi.  One rotation: every lane l updates G[l][p], G[l][q] and their mirror
// images G[p][l], G[q][l] (lane p instead writes the rotated 2 x 2 block), and V[l][p], V[l][q].  No lane reads what another writes
// within a rotation; wave_sync() orders one rotation's stores before the next one's loads.  Returns true if a sweep skipped
// every rotation within FIT_MAX_SWEEPS.
template <int NZ, int PITCH>
__device__ __forceinline__ bool fit_jacobi(cplx* G, cplx* V, int lane) {
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  if (act) {
#pragma unroll 1
    for (int i = 0; i < NZ; ++i) V[i * PITCH + l] = mk(i == l ? 1.0 : 0.0, 0.0);
  }
#pragma unroll 1
  for (int sweep = 0; sweep < FIT_MAX_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll 1
    for (int p = 0; p < NZ - 1; ++p) {
#pragma unroll 1
      for (int q = p + 1; q < NZ; ++q) {
        wave_sync();
        const cplx g = G[p * PITCH + q];
        const double app = G[p * PITCH + p].re, aqq = G[q * PITCH + q].re;
        const double m2 = g.re * g.re + g.im * g.im;
        if (uniform(m2 <= FIT_EPS * FIT_EPS * fabs(app * aqq))) continue;
        rotated = true;
        const double absg = sqrt(m2);
        const double tau = (aqq - app) / (2.0 * absg);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t);
        const cplx sw = mk(t * c * (g.re / absg), t * c * (g.im / absg));
        cplx gp, gq, vp, vq;
        rotate_pair(c, sw, G[l * PITCH + p], G[l * PITCH + q], gp, gq);
        rotate_pair(c, sw, V[l * PITCH + p], V[l * PITCH + q], vp, vq);
        if (act) {
          if (l == p) {
            G[p * PITCH + p] = mk(app - t * absg, 0.0);
            G[q * PITCH + q] = mk(aqq + t * absg, 0.0);
            G[p * PITCH + q] = czero();
            G[q * PITCH + p] = czero();
          } else if (l != q) {
            G[l * PITCH + p] = gp;
            G[l * PITCH + q] = gq;
            G[p * PITCH + l] = cconj(gp);
            G[q * PITCH + l] = cconj(gq);
          }
          V[l * PITCH + p] = vp;
          V[l * PITCH + q] = vq;
        }
      }
    }
    if (!rotated) return true;
  }
  return false;
}

// Singular values: s_k = sqrt(sum over the snapshots of |v_k^H z|^2), the Rayleigh quotient v_k^H G v_k taken from the data
// themselves in a second pass over them, lane l on column l of V; every term is non-negative, so a singular value that is zero
// comes out at the rounding of the inner products (~eps s_0), not at sqrt of the rounding floor of G (~1e-8 s_0).  Stored in
// descending order by rank-counting in LDS (Z's place).  ok = false: zeros.
// REFIT: the sums of the weighted stack, by G's recurrence: only t < steps, s2 <- d2 s2 (a product of its own) before a term is added.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ void fit_svals(const FitArgs& a, long b, cplx* lds, int lane, bool ok, const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  const cplx* V = lds + L::V;
  const cplx* Z = lds + L::Z;
  double* S2 = reinterpret_cast<double*>(lds + L::Z);
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  if (!uniform(ok)) {
    if (act) gst(a.svals, b * NZ + l, 0.0);
    return;
  }
  double s2 = 0.0;
  [[maybe_unused]] const double d2 = pr.discount * pr.discount;
  [[maybe_unused]] int t = 0;
  fit_stream<NX, NU, ORDER>(a, b, lds, lane, [&](cplx) {
    if constexpr (REFIT) {
      const bool taken = uniform(t < pr.steps);
      if (++t == a.N) t = 0;
      if (!taken) return;
      s2 *= d2;
      asm volatile("" : "+v"(s2));       // (rounded before the add: the empty asm keeps the two from contracting into an FMA)
    }
    cplx d = czero();
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) cmac_cj(d, V[j * PITCH + l], Z[j]);      // += conj(V[j][l]) z_j
    s2 += d.re * d.re + d.im * d.im;
  });
  if (act) S2[l] = s2;
  wave_sync();
  int pos = 0;
#pragma unroll 1
  for (int k = 0; k < NZ; ++k) {
    const double sk = S2[k];
    pos += (sk > s2 || (sk == s2 && k < l)) ? 1 : 0;
  }
  if (act) gst(a.svals, b * NZ + pos, sqrt(s2));
  wave_sync();
}

// The truncated products of phase 3, shared with the QR route (m4q_fit_qr.h): C holds W[:, k] / lam_k, LAM the spectrum and lmax
// its maximum; per rcond A = sum_{lam_k > rcond^2 lmax} C[:, k] V[:, k]^H, lane l on column l of A.  ok = false: zero models and ranks.
// REFIT: A0 is added to every entry of the finished sum.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ void fit_truncate(const FitArgs& a, long b, cplx* lds, int lane, bool ok, double lmax,
                                             const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  const cplx* V = lds + L::V;
  const cplx* C = lds + L::C;
  const double* LAM = reinterpret_cast<const double*>(lds + L::LAM);
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  cplx acc[NX];
  for (int r = 0; r < a.R; ++r) {
    const double rc = gld(a.rconds, r);
    const double thr = (rc * rc) * lmax;
    int rank = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = czero();
    if (uniform(ok)) {
#pragma unroll 1
      for (int k = 0; k < NZ; ++k) {
        if (!uniform(LAM[k] > thr)) continue;
        ++rank;
        const cplx v = cconj(V[l * PITCH + k]);
#pragma unroll
        for (int i = 0; i < NX; ++i) cmac(acc[i], C[i * PITCH + k], v);
      }
      if constexpr (REFIT) {
#pragma unroll
        for (int i = 0; i < NX; ++i) acc[i] = cadd(acc[i], gld(pr.A0, i * NZ + l));
      }
    }
    const long m0 = ((long)r * a.B + b) * NX * NZ;
    if (act) {
#pragma unroll
      for (int i = 0; i < NX; ++i) gst(a.models, m0 + i * NZ + l, acc[i]);
    }
    if (lane == 0 && a.ranks) gst(a.ranks, (long)r * a.B + b, rank);
  }
}

// Phase 3: eigenvalues, then per rcond the truncated product
// A = sum_{lam_k > rcond^2 max(lam)} (W[:, k] / lam_k) V[:, k]^H with W = C V; lane l holds column l of A and stores it along the nz
// axis (coalesced).  ok = false: zero models and ranks.
template <int NX, int NU, int ORDER, bool REFIT = false>
__device__ __forceinline__ void fit_models(const FitArgs& a, long b, cplx* lds, int lane, bool ok, const FitPrior& pr = FitPrior{}) {
  using L = FitLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  cplx* G = lds + L::G;
  cplx* V = lds + L::V;
  cplx* C = lds + L::C;
  double* LAM = reinterpret_cast<double*>(lds + L::LAM);
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  cplx acc[NX];
  wave_sync();
  const double lam_l = G[l * PITCH + l].re;
  if (act) LAM[l] = lam_l;
  wave_sync();
  double lmax = LAM[0];
#pragma unroll 1
  for (int k = 1; k < NZ; ++k) lmax = fmax(lmax, LAM[k]);
  if (uniform(ok)) {
#pragma unroll
    for (int i = 0; i < NX; ++i) acc[i] = czero();
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) {
      const cplx v = V[j * PITCH + l];
#pragma unroll
      for (int i = 0; i < NX; ++i) cmac(acc[i], C[i * PITCH + j], v);
    }
    wave_sync();
    const double inv = 1.0 / lam_l;
    if (act) {
#pragma unroll
      for (int i = 0; i < NX; ++i) C[i * PITCH + l] = cscale(acc[i], inv);
    }
    wave_sync();
  }
  fit_truncate<NX, NU, ORDER, REFIT>(a, b, lds, lane, ok, lmax, pr);
}

}  // namespace m4q

// m4q_online.h - device functions of online_dmdc_kernel (m4q_kernels.hip): the recursive least-squares update of a DMDc model
// with a forgetting factor (model.py: OnlineDMDc.fit_iteration) for every snapshot of a member, m4q_online_dmdc_batch.
// mpc4quantum_amd/online.py (online_dmdc_reference) is the definition; what is here follows it operation by operation, so the two
// differ only by the device's division and the compiler's FMA contraction.
//
// The frame is dmdc_fit_kernel's (m4q_fit.h): ONE WAVEFRONT OWNS ONE MEMBER, lane l owns index l of the nz axis, the snapshots come
// in through its fit_stream.  The state P [nz][PITCH] and A [n][PITCH] (PITCH = nz | 1, as there) stays in LDS from the first
// snapshot to the last, beside the vectors one update passes between lanes: z [nz], y = x_{t+1} [n], gamma Pz [nz], w [nz], r [n]
// and gamma r [n].  Lane l reads ROW l of P for (P z)_l and owns COLUMN l of P and A in the rank-one updates (w_l stays in its
// registers), so no lane writes what another one reads between two wave_sync().  All control flow is wave-uniform.
#pragma once
#include "m4q_fit.h"

namespace m4q {

template <int NX, int NU, int ORDER>
struct OnlineLayout {
  static constexpr int NZ = NX * (1 + PowTab<NU, ORDER>::NP);
  static constexpr int PITCH = NZ | 1;
  // offsets in cplx elements
  static constexpr int P = 0, A = P + NZ * PITCH, Z = A + NX * PITCH, XN = Z + NZ, PZ = XN + NX, W = PZ + NZ, R = W + NZ, GR = R + NX;
  static constexpr int ELEMS = GR + NX;
  static constexpr size_t BYTES = sizeof(cplx) * (size_t)ELEMS;
  static constexpr bool FITS = NZ <= 64 && BYTES <= FIT_LDS_LIMIT;
};

__device__ __forceinline__ bool finite_c(cplx a) { return finite_d(a.re) && finite_d(a.im); }

// A = A0[b], P = P0[b] (or alpha I) into LDS, lane l its column
template <int NX, int NU, int ORDER>
__device__ __forceinline__ void online_load(const OnlineArgs& a, long b, cplx* lds, int lane) {
  using L = OnlineLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  cplx* P = lds + L::P;
  cplx* A = lds + L::A;
  if (lane < NZ) {
    const M4Q_GLOBAL cplx* a0 = a.A0 + b * a.A0_stride;
#pragma unroll
    for (int i = 0; i < NX; ++i) A[i * PITCH + lane] = gld(a0, i * NZ + lane);
    if (a.P0) {
      const M4Q_GLOBAL cplx* p0 = a.P0 + b * a.P0_stride;
#pragma unroll 1
      for (int i = 0; i < NZ; ++i) P[i * PITCH + lane] = gld(p0, i * NZ + lane);
    } else {
#pragma unroll 1
      for (int i = 0; i < NZ; ++i) P[i * PITCH + lane] = mk(i == lane ? a.alpha : 0.0, 0.0);
    }
  }
  wave_sync();
}

// Every snapshot of member b in its order: one update of (A, P) for each of the first `steps` of every experiment (online.py, in
// its order of operations); the others stream past.  Returns false if a snapshot taken held a non-finite entry.
template <int NX, int NU, int ORDER, bool HERM>
__device__ __forceinline__ bool online_updates(const OnlineArgs& a, long b, int steps, double inv_discount, cplx* lds, int lane) {
  using L = OnlineLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  cplx* P = lds + L::P;
  cplx* A = lds + L::A;
  const cplx* Z = lds + L::Z;
  const cplx* XN = lds + L::XN;
  cplx* PZ = lds + L::PZ;
  cplx* W = lds + L::W;
  cplx* R = lds + L::R;
  cplx* GR = lds + L::GR;
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  const int lx = lane < NX ? lane : NX - 1;
  const int N = a.N;
  bool ok = true;
  int t = 0, e = 0, records = 0, until_record = a.hist_every;
  fit_stream<NX, NU, ORDER, L>(a, b, lds, lane, [&](cplx z) {
    if (!uniform(t < steps)) {                           // beyond the member's count: the snapshot streams past, nothing is taken
      if (++t == N) { t = 0; ++e; }
      return;
    }
    ok = ok && finite_c(z) && finite_c(XN[lx]);
    // (P z)_l along row l; w_l = (P z)_l, or - the conjugated form - sum_i conj(z_i) P[i][l] down column l; r_i on lanes i < n
    cplx pz = czero(), w = czero(), r = XN[lx];
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) {
      const cplx zj = Z[j];
      cmac(pz, P[l * PITCH + j], zj);
      if (HERM) cmac_cj(w, zj, P[j * PITCH + l]);        // += conj(z_j) P[j][l]
      cmsub(r, A[lx * PITCH + j], zj);
    }
    if (!HERM) w = pz;
    if (act) W[l] = w;
    if (lane < NX) R[lane] = r;
    wave_sync();
    cplx s = czero();
#pragma unroll 1
    for (int j = 0; j < NZ; ++j) cmac(s, W[j], Z[j]);
    const double dre = 1.0 + s.re, dim = s.im;
    const double den = dre * dre + dim * dim;
    const cplx gamma = mk(dre / den, -dim / den);
    double innov = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const cplx ri = R[i];
      innov += ri.re * ri.re + ri.im * ri.im;
    }
    if (a.innov && lane == 0) gst(a.innov, (b * a.E + e) * (long)N + t, innov);
    if (act) PZ[l] = cmul(gamma, pz);
    if (lane < NX) GR[lane] = cmul(gamma, r);
    wave_sync();
    if (act) {
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        cplx v = A[i * PITCH + l];
        cmac(v, GR[i], w);
        A[i * PITCH + l] = v;
      }
#pragma unroll 1
      for (int i = 0; i < NZ; ++i) {
        cplx v = P[i * PITCH + l];
        cmsub(v, PZ[i], w);
        P[i * PITCH + l] = cscale(v, inv_discount);
      }
    }
    if (a.hist && --until_record == 0) {                 // (the host passes hist only with hist_every > 0)
      until_record = a.hist_every;
      const long h0 = ((long)records++ * a.B + b) * NX * NZ;
      if (act) {
#pragma unroll
        for (int i = 0; i < NX; ++i) gst(a.hist, h0 + i * NZ + l, A[i * PITCH + l]);
      }
    }
    if (++t == N) { t = 0; ++e; }
  });
  return !__any(!ok);
}

// The member's outputs: A, P (when wanted) and the status; zeros for a member whose data or final state is not finite, in the
// records of `hist` as well; the records and the innovations the member never reached are zero.
template <int NX, int NU, int ORDER>
__device__ __forceinline__ void online_store(const OnlineArgs& a, long b, int steps, bool data_ok, const cplx* lds, int lane) {
  using L = OnlineLayout<NX, NU, ORDER>;
  constexpr int NZ = L::NZ, PITCH = L::PITCH;
  const cplx* P = lds + L::P;
  const cplx* A = lds + L::A;
  const bool act = lane < NZ;
  const int l = act ? lane : NZ - 1;
  bool fin = data_ok;
#pragma unroll
  for (int i = 0; i < NX; ++i) fin = fin && finite_c(A[i * PITCH + l]);
#pragma unroll 1
  for (int i = 0; i < NZ; ++i) fin = fin && finite_c(P[i * PITCH + l]);
  const bool ok = !__any(!fin);
  if (act) {
#pragma unroll
    for (int i = 0; i < NX; ++i) gst(a.models, (b * NX + i) * NZ + l, ok ? A[i * PITCH + l] : czero());
    if (a.P) {
#pragma unroll 1
      for (int i = 0; i < NZ; ++i) gst(a.P, (b * NZ + i) * NZ + l, ok ? P[i * PITCH + l] : czero());
    }
  }
  if (a.hist) {
    const int H = (a.E * a.N) / a.hist_every;
    const int written = ok ? (a.E * steps) / a.hist_every : 0;
    for (int h = written; h < H; ++h) {
      const long h0 = ((long)h * a.B + b) * NX * NZ;
      if (act) {
#pragma unroll
        for (int i = 0; i < NX; ++i) gst(a.hist, h0 + i * NZ + l, czero());
      }
    }
  }
  if (a.innov) {
    for (int e = 0; e < a.E; ++e)
      for (int t = steps + lane; t < a.N; t += 64) gst(a.innov, (b * a.E + e) * (long)a.N + t, 0.0);
  }
  if (lane == 0) gst(a.status, b, ok ? 0 : 3);
}

}  // namespace m4q

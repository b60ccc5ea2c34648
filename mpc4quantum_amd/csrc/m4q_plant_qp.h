// m4q_plant_qp.h - the QP of m4q_quad_program_batch posed on the plant's own linearisation without the host in between
// (m4q_plant_quad_program_batch; mpc4quantum_amd/plant_linearize.py: plant_quad_program_reference is the definition).
//
// A_t = (U_t (x) U_t^*) (x) I_NC is fully described by the d x d propagator U_t (m4q_plant_lin.h): the factor kernel leaves U_t,
// B_t and Delta_t in device workspaces, and the provider below forms the column and the row of A_t a lane owns from 2 d entries of
// U_t instead of reading n entries of A_t.  Every entry is formed, the delta(c, c') zeros included, by plant_lin_entry's operation
// and summed in ExplicitProv's order, so the numbers follow m4q_plant_linearize_batch + m4q_quad_program_batch.
#pragma once
#include "m4q_mpc.h"
#include "m4q_plant_lin.h"

namespace m4q {

// ExplicitProv's interface on (U_t, B_t, Delta_t).  State index i = (a, e, c): i = (a D + e) NC + c.
template <int NX, int NU, int D, int NC>
struct PlantProv {
  static_assert(D * D * NC == NX, "state is a vectorised d x d matrix, or d^2 columns of them");
  static constexpr int ORDER_ = 1;   // (the QP kernels do not depend on the library order)
  GView U_ls;   // [T][D][D]     positioned at this instance
  GView B_ls;   // [T][NX][NU]
  GView D_ls;   // [T][NX]
  int j;
  struct Lin {
    int t;
  };
  __device__ __forceinline__ Lin fetch(int t) const { Lin l; l.t = t; return l; }
  // column j = (g, h, c') of A_t: U[:, g] and U[:, h]
  __device__ __forceinline__ void col(const Lin& l, cplx (&Ac)[NX]) const {
    const int rc = j / NC, cc = j - rc * NC;
    const int g = rc / D, h = rc - g * D;
    cplx ug[D], uh[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      ug[a] = U_ls.ld<cplx>((l.t * D + a) * D + g);
      uh[a] = U_ls.ld<cplx>((l.t * D + a) * D + h);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int ri = i / NC, ci = i - ri * NC;
      const int a = ri / D, e = ri - a * D;
      Ac[i] = csel(ci == cc, cmul(ug[a], cconj(uh[e])), czero());
    }
  }
  __device__ __forceinline__ void col_rows(const Lin& l, cplx v, cplx (&Ac)[NX], cplx& av, cplx (&Brow)[NU], cplx& dlt) const {
    col(l, Ac);
    rows(l, v, av, Brow, dlt);
  }
  __device__ __forceinline__ void brows(const Lin& l, cplx (&Brow)[NU]) const {
#pragma unroll
    for (int k = 0; k < NU; ++k) Brow[k] = B_ls.ld<cplx>((l.t * NX + j) * NU + k);
  }
  // row j = (a, e, c) of A_t: U[a, :] and U[e, :]
  __device__ __forceinline__ void rows(const Lin& l, cplx v, cplx& av, cplx (&Brow)[NU], cplx& dlt) const {
    const int ri = j / NC, ci = j - ri * NC;
    const int a = ri / D, e = ri - a * D;
    cplx ua[D], ue[D];
#pragma unroll
    for (int g = 0; g < D; ++g) {
      ua[g] = U_ls.ld<cplx>((l.t * D + a) * D + g);
      ue[g] = U_ls.ld<cplx>((l.t * D + e) * D + g);
    }
    cplx arow[NX];
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int rc = k / NC, cc = k - rc * NC;
      const int g = rc / D, h = rc - g * D;
      arow[k] = csel(ci == cc, cmul(ua[g], cconj(ue[h])), czero());
    }
    av = dot_lane_index<false, false, NX>(v, arow);
#pragma unroll
    for (int k = 0; k < NU; ++k) Brow[k] = B_ls.ld<cplx>((l.t * NX + j) * NU + k);
    dlt = D_ls.ld<cplx>(l.t * NX + j);
  }
};

}  // namespace m4q

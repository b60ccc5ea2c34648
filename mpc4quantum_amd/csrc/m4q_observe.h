// m4q_observe.h - observed plants: the loop sees x = observe(z) of a plant state z that it does not model (observe.py is the
// definition; the kernels are in the auxiliary section of m4q_kernels.hip).
//   OBSERVE_PARTIAL_TRACE  z = vec_r of a two-qubit state (n_p = 16), x = [vec_r(tr_B rho), vec_r(tr_A rho)] (n = 8)
//                          (QCoupledExperiment.lift, experiment.py:238-306)
//   OBSERVE_QUBIT_BLOCK    z = vec_r of a three-level state (n_p = 9), x = vec_r(Bk / |Bk|_tr) with Bk its leading 2 x 2 block
//                          (n = 4; QExperiment32.lift, experiment.py:215-235)
// One DPP row per member, as everywhere; the lane geometry is on n_p - the plant state - not on the NX of the shape whose object
// holds the kernel: lane jj < n_p owns z[jj], lane jj < n forms and stores x[jj].
#pragma once
#include "m4q_args.h"
#include "m4q_mpc.h"

namespace m4q {

template <int OBS> struct ObserveDims;
template <> struct ObserveDims<OBSERVE_PARTIAL_TRACE> { static constexpr int NP = 16, DP = 4, N = 8; };
template <> struct ObserveDims<OBSERVE_QUBIT_BLOCK> { static constexpr int NP = 9, DP = 3, N = 4; };
// LDS of one row of observed_plant_kernel (complex elements): the plant step's scratch (m4q_mpc.h: plant_hamiltonian); the
// observation goes through its first n_p elements
template <int OBS>
constexpr int observe_row_elems() { return ObserveDims<OBS>::DP * ObserveDims<OBS>::DP + 2 * ObserveDims<OBS>::NP; }

// geometry of one lane inside its quad, on a plant state of NPL entries (LaneGeo of m4q_kernels.hip is on the shape's NX)
template <int NPL>
struct PlantLaneGeo {
  int g, jj, j;
  __device__ __forceinline__ PlantLaneGeo() {
    const int lane = threadIdx.x;
    g = lane >> 4;
    jj = lane & 15;
    j = jj < NPL ? jj : NPL - 1;
  }
};

// x[jj] = observe(z)[jj] for the row whose lane jj < n_p holds z[jj]; blk: n_p complex of the row's LDS.  Lanes jj >= n return
// a value nobody stores.  One wavefront per workgroup: wave_sync is the wave's own LDS fence; the block is free again on return.
template <int OBS>
__device__ __forceinline__ cplx observe_row(cplx z, cplx* blk, int jj) {
  constexpr int NPL = ObserveDims<OBS>::NP, NO = ObserveDims<OBS>::N;
  if (jj < NPL) blk[jj] = z;
  wave_sync();
  const int e = jj < NO ? jj : NO - 1;
  cplx x;
  if constexpr (OBS == OBSERVE_PARTIAL_TRACE) {
    // r[a][b][a'][b'] = z[(2a + b) 4 + 2a' + b']
    const int h = e & 3, p = h >> 1, q = h & 1;
    // e < 4: x[2a + a'] = r[a][0][a'][0] + r[a][1][a'][1];  else x[4 + 2b + b'] = r[0][b][0][b'] + r[1][b][1][b']
    const int i0 = e < 4 ? 8 * p + 2 * q : 4 * p + q;
    const int i1 = e < 4 ? i0 + 5 : i0 + 10;
    x = cadd(blk[i0], blk[i1]);
  } else {
    const cplx b00 = blk[0], b01 = blk[1], b10 = blk[3], b11 = blk[4];
    double f2 = norm2(b00);
    f2 += norm2(b01);
    f2 += norm2(b10);
    f2 += norm2(b11);
    const cplx det = csub(cmul(b00, b11), cmul(b01, b10));
    const double s = sqrt(f2 + 2.0 * sqrt(norm2(det)));           // the trace norm s1 + s2 of the block (observe.py)
    const cplx me = blk[(e >> 1) * 3 + (e & 1)];
    x = mk(me.re / s, me.im / s);                                 // s = 0: NaN, as the reference's 0 / 0
  }
  wave_sync();
  return x;
}

}  // namespace m4q

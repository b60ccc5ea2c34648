// m4q_rollout_multi.h - S control sequences shared by the ensemble, each rolled against all B members in ONE launch
// (m4q_plant_rollout_multi_batch; the line search of m4q_plant_robust_batch, whose candidates of one iteration are such a set).
// What a pulse optimised against an ensemble asks of a candidate is one number, F[s] = sum_b w_b J[b][s]: this kernel leaves the
// members' objectives J [B][S] and stores no state; the ordered reduction behind it (grad_reduce_kernel, m4q_grad.h) forms F.
//
// Included by m4q_kernels.hip inside its shape namespace, behind plant_rollout_grad_kernel: the kernel is written on that file's
// NX, NU, LaneGeo, QuadRow, quad_figure and M4Q_PLANT_STEP.  The step is the device function plant_rollout_kernel calls, on operands
// formed as that kernel forms them (u_scale[b][k] us[s][t][k] in fp64, dts[t]), and q_t is RollOut's quad_figure of x_t - f against
// row j of W: J[b][s] has the bits of m4q_plant_rollout_batch's figure under us[s] - q_N (q_mode 1), or its N + 1 columns added
// with t ascending from 0.0 (q_mode 2; grad.py: _reference adds them so).
//
// One DPP row per member, launch_aux's grid over quads of members.  A row loads its member's x0, u_scale and target entry once and
// forms its operator views once; pass s then rolls us[s] from x0 with the state in registers.  The controls and the interval of
// step t + 1 are fetched while step t computes (they are the same in every lane of the wavefront: one address per load).
// A row past the end of the ensemble repeats the last member's reads and stores nothing.

template <int PLANT>
__global__ __launch_bounds__(64) M4Q_OCC void plant_rollout_multi_kernel(MultiArgs a) {
  static_assert(PLANT == PLANT_HAMILTONIAN || PLANT == PLANT_PROCESS, "the generator plant's kernels live in the other object");
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* scratch = lds + g * SCRATCH_ELEMS;
  const int nquads = quads_of(a.B);
  const M4Q_GLOBAL cplx* Wr = a.W + j * NX;          // row j of W
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    const GView op0 = gview(a.plant.op0, r.q0 * a.plant.op0_stride, r.gl * (unsigned)a.plant.op0_stride);
    const GView ops = gview(a.plant.ops, r.q0 * a.plant.ops_stride, r.gl * (unsigned)a.plant.ops_stride);
    const bool st0 = r.valid && jj == 0;
    double sc[NU];
#pragma unroll
    for (int k = 0; k < NU; ++k) sc[k] = a.u_scale ? gld(a.u_scale, r.b * NU + k) : 1.0;
    const cplx x0 = gld(a.x0, r.b * NX + j);
    const cplx f = gld(a.target, r.b * a.target_stride + j);
    for (int s = 0; s < a.S; ++s) {
      const M4Q_GLOBAL double* u = a.us + (long)s * a.N * NU;
      double un[NU];
#pragma unroll
      for (int k = 0; k < NU; ++k) un[k] = gld(u, k);
      double dtn = gld(a.dts, 0);
      cplx x = x0;
      double J = 0.0;
      if (a.q_mode == 2) J = J + quad_figure<NX>(csub(x, f), Wr);
      for (int t = 0; t < a.N; ++t) {
        const int tn = t + 1 < a.N ? t + 1 : t;
        double v[NU];
#pragma unroll
        for (int k = 0; k < NU; ++k) {
          v[k] = sc[k] * un[k];
          un[k] = gld(u, (long)tn * NU + k);
        }
        const double dt = dtn;
        dtn = gld(a.dts, tn);
        M4Q_PLANT_STEP(PLANT, x, x, v, op0, ops, dt, scratch, j, jj);
        if (a.q_mode == 2) J = J + quad_figure<NX>(csub(x, f), Wr);
      }
      if (a.q_mode != 2) J = quad_figure<NX>(csub(x, f), Wr);
      if (st0) gst(a.J, r.b * a.S + s, J);
    }
  }
}

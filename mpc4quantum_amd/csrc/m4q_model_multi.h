// m4q_model_multi.h - S control sequences shared by the ensemble, each rolled through all B members' MODELS in ONE launch
// (m4q_model_rollout_multi_batch; the line search of m4q_model_robust_batch).  The model-side twin of m4q_rollout_multi.h: the
// kernel leaves the members' objectives J [B][S] and stores no state; the ordered reduction behind it (grad_reduce_kernel,
// m4q_grad.h) forms F[s] = sum_b w_b J[b][s].
//
// Included by m4q_kernels.hip inside its shape namespace, behind model_rollout_grad_kernel: the kernel is written on that file's
// NX, NU, ORDER, NP, LaneGeo, QuadRow, stage_model and quad_figure.  The step performs the operations of FusedProv::rows' complex
// path for (A_t x)_j in their order, column by column with k ascending: own = A[j][k], then cmac_r by po.pu[p] with p ascending,
// then ONE broadcast term acc += lane_k(x) own - re re, re im, -im im, im re: the sequence rows' column-wise statement
// (emit_terms<IdxSameLaneVec<k>>) gives each of its accumulators.  dot_lane_index over a finished row is another sequence - a dot
// statement adds the re re products of its four terms before their -im im products - and rounds differently.
// The controls are formed as RollCtl::take forms them (u_scale[b][k] us[s][t][k] in fp64),
// and q_t is RollOut's quad_figure of x_t - f against row j of W: J[b][s] has the bits of m4q_model_rollout_batch's figure under
// us[s] - q_N (q_mode 1), or its N + 1 columns added with t ascending from 0.0 (q_mode 2; grad.py: _reference adds them so).
// Of rows' outputs only A_t x is formed: row j of B_t and Delta_t are not needed by a rollout.
//
// One DPP row per member, launch_aux's grid over quads of members.  The member's model (or the shared one, model_stride 0) is
// staged once per quad; x0, u_scale and the target entry are loaded once per member.  What model_rollout_kernel reads from LDS at
// every step - the lane's (1 + NP) NX row entries, which depend neither on s nor on t - is loaded into registers ONCE per member
// where that fits (MULTI_ROWS_IN_REGS), and all S N steps then run from registers; elsewhere the rows are read from LDS per step.
// A row past the end of the ensemble repeats the last member's reads and stores nothing.

// The lane's rows take 4 (1 + NP) NX VGPRs: 32 at (4, 1, 1), 48 at (4, 1, 2) and (4, 2, 1), 96 at (8, 2, 1), 108 at (9, 2, 1).
// Beyond that - 192 at (16, 1, 2), 216 at (9, 2, 2), 256 and more at (16, 3, 1) and (16, 1, 3..4) - they do not fit beside the
// step's own registers without spilling; (16, 1, 1), 128 VGPRs at one wavefront per SIMD, is decided with them.
#if defined(M4Q_DEV_MULTI_LDS)
constexpr bool MULTI_ROWS_IN_REGS = false;           // (development builds: the LDS form everywhere, to time one against the other)
#else
constexpr bool MULTI_ROWS_IN_REGS = 4 * (1 + NP) * NX <= 128;
#endif

// the lane's rows of the model's blocks: rows.v[p][k] = block p, element [j][k]
template <bool REGS>
struct MultiRows {
  cplx v[REGS ? 1 + NP : 1][REGS ? NX : 1];
  const cplx* mdl;
  int j, off;
  __device__ __forceinline__ void load(const cplx* mdl_, int j_) {
    mdl = mdl_; j = j_; off = 0;
    if constexpr (REGS) {
#pragma unroll
      for (int p = 0; p <= NP; ++p) {
#pragma unroll
        for (int k = 0; k < NX; ++k) v[p][k] = mld(mdl, ModelPitch<NX>::at(p, j, k));
      }
    }
  }
  __device__ __forceinline__ cplx el(int p, int k) const {
    if constexpr (REGS) return v[p][k];
    else return mld(mdl, ModelPitch<NX>::at(p, j, k) + off);
  }
  // The LDS form, once per step: an offset of zero through an opaque asm, so that the reads - invariants of the step loop - stay
  // in the step that uses them (hoisted out of the loop they are the register form again, and spill where that form does not fit;
  // the block's address itself stays what the compiler knows to be LDS)
  __device__ __forceinline__ void step() {
    if constexpr (!REGS) asm volatile("" : "+v"(off));
  }
};

__global__ __launch_bounds__(64) M4Q_OCC void model_rollout_multi_kernel(ModelMultiArgs a) {
  cplx* lds = reinterpret_cast<cplx*>(m4q_lds_raw);
  const LaneGeo L;
  const int g = L.g, jj = L.jj, j = L.j;
  cplx* mdl = lds + g * MODEL_ELEMS;
  const int nquads = quads_of(a.B);
  const M4Q_GLOBAL cplx* Wr = a.W + j * NX;          // row j of W
  for (int quad = blockIdx.x; quad < nquads; quad += gridDim.x) {
    const QuadRow r(quad, g, a.B);
    wave_sync();
    stage_model<NX>(mdl, a.models + r.b * a.model_stride, jj);
    wave_sync();
    MultiRows<MULTI_ROWS_IN_REGS> rows;
    rows.load(mdl, j);
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
        Poly<NU, ORDER> po;
        po.eval(v);
        rows.step();
        cplx xn = czero();
        static_for<0, NX>([&](auto kk) {
          constexpr int k = decltype(kk)::value;
          cplx own = rows.el(0, k);
#pragma unroll
          for (int p = 0; p < NP; ++p) cmac_r(own, rows.el(1 + p, k), po.pu[p]);
          cmac_bc<k>(xn, x, own);                            // xn += lane_k(x) (A + sum_p polyu_p N_p)[j][k]
        });
        x = xn;
        if (a.q_mode == 2) J = J + quad_figure<NX>(csub(x, f), Wr);
      }
      if (a.q_mode != 2) J = quad_figure<NX>(csub(x, f), Wr);
      if (st0) gst(a.J, r.b * a.S + s, J);
    }
  }
}

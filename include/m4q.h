/* m4q.h - C ABI of libm4q_hip.so: batched receding-horizon MPC for quantum state preparation on
 * AMD MI355X (gfx950).  This is the drop-in boundary for the hot path of andgoldschmidt/MPC4quantum.
 *
 * The reference has no FFI: its boundary for this path is three Python call signatures
 * (citations into the reference tree):
 *     mpc4quantum/mpc.py:128-129       mpc(x0, dim_u, order, X_targ, U_targ, clock, experiment, model, Q, R, Qf, ...)
 *     mpc4quantum/optimize.py:12       quad_program(x_init, X_bm, U_bm, Q_ls, R_ls, A_ls, B_ls, Delta_ls, u_prev, sat, du)
 *     mpc4quantum/linearize.py:61-70   WrapModel.get_model_along_traj(xs, us, ts)
 * and the plant call  mpc4quantum/experiment.py:202-212  QExperiment.simulate(x0, ts, us).
 * Each entry point below names the reference interface it replaces.  mpc4quantum_amd/ binds them
 * with ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - complex numbers are interleaved (re, im) doubles; all arithmetic is fp64;
 *   - every array is C-contiguous with the ENSEMBLE AXIS OUTERMOST and TIME before state:
 *       trajectories  X[b][t][i]   (the reference holds one instance as X[i][t]);
 *   - a model is the reference's DMDc.A block matrix, A[b][i][p*n + k], n x n(1+P) (model.py:95-103,
 *     column layout of linearize.krtimes, linearize.py:80-89); P = number of non-constant control
 *     monomials of the library of the given order (linearize.py:113-120);
 *   - "*_per_instance" = 0 means one array shared by the whole ensemble (no leading b axis);
 *   - host entry points (m4q_*_batch) take caller-owned HOST buffers, copy, launch, copy back;
 *     the session API keeps everything resident in HBM;
 *   - return value: 0 on success, a negative number on failure (-hipError_t for runtime errors,
 *     M4Q_E_* otherwise); m4q_last_error() gives the message.  One host thread per session.
 */
#ifndef M4Q_H
#define M4Q_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define M4Q_API __attribute__((visibility("default")))
#else
#define M4Q_API
#endif

#define M4Q_E_UNSUPPORTED (-1001) /* (dim_x, dim_u, order) has no compiled kernel */
#define M4Q_E_BADARG (-1002)
#define M4Q_E_NODEVICE (-1003)
#define M4Q_E_TIMEOUT (-1004) /* the closed-loop launch abandoned itself: its watchdog (M4Q_KERNEL_TIMEOUT_S, default 300 s of device
                                 time) expired before every member had finished; results of that launch are not valid */

/* qp_flags */
#define M4Q_QP_REF_LQR 1 /* reproduce mpc4quantum/lqr.py:14-79 as written (no Delta, no du band) */
#define M4Q_QP_DU_BAND 2 /* also clip the first control to u_prev +- du (optimize.py:29-30) */
#define M4Q_QP_EXACT_BOX 4 /* solve the box-constrained QP of optimize.py:27-54 to optimality (projected Newton on the
                              Riccati factorisation) instead of clipping the unconstrained rollout; not with
                              M4Q_QP_REF_LQR */

/* plant_kind */
#define M4Q_PLANT_NONE 0        /* caller supplies xs[step+1] between m4q_session_run calls */
#define M4Q_PLANT_HAMILTONIAN 1 /* rho+ = U rho U^H, U = expm(-i dt (H0 + sum_k u_k H_k)), d x d operators */
#define M4Q_PLANT_GENERATOR 2   /* x+ = expm(dt (L0 + sum_k u_k L_k)) x, n x n operators */
/* gate synthesis (experiment.py:336-417, QSynthesis): x = vec_r(M) is the process vector of a d x d unitary, M = U (x) U^* a
 * d^2 x d^2 matrix, n = d^4 (a qubit gate: d = 2, n = 16).  x+ = vec_r((V (x) V^*) M), V = expm(-i dt (H0 + sum_k u_k H_k)), d x d
 * operators.  The loop state is the process vector itself (no lift).  Sessions with this plant always run the complex path
 * (m4q_session_path 0): V (x) V^* does not keep M Hermitian.  M4Q_E_BADARG if n is not a fourth power. */
#define M4Q_PLANT_PROCESS 3

/* options (m4q_problem.reserved).  By default a session whose model, states, targets and costs are real in a
 * Hermitian operator basis (every vectorised-Liouvillian model and Hermitian state is) runs the closed loop in
 * that basis with real arithmetic - a quarter of the flops of the complex recursion of lqr.py, same results to
 * rounding; anything else runs the general complex path.  This bit forces the complex path. */
#define M4Q_OPT_FORCE_COMPLEX 1
/* A real-path session whose model also leaves the identity component of rho alone (trace-preserving and unital: every
 * vectorised Liouvillian -i[H, .] and its Taylor truncation) and whose initial states and targets share one trace runs the
 * recursion on the d*d - 1 traceless Hermitian coordinates - one dimension fewer, same results to rounding.  This bit keeps
 * such a session on the d*d-coordinate real path. */
#define M4Q_OPT_NO_TRACELESS 2
/* A traceless session with a constant target over the horizon window runs the BACKWARD sweep of the clipped solve on fp64
 * matrix-core tiles (v_mfma_f64_4x4x4_4b_f64: one member per 16-lane block, its operands fetched four horizon indices at a time,
 * csrc/m4q_tile3.h) and the rollout on DPP rows, wherever that form is built: d = 2 and d = 3 (3 and 8 traceless coordinates: at
 * d = 3 the DPP layout leaves half of every row idle) with an order-1 model.  Same results to rounding; config 3 35.5 -> 29.9 ms,
 * config 2 4.05 -> 2.9 ms, config 5's share 117.8 -> 104.4 ms (profiles/r04_ab_experiments.txt).  At d = 4 the DPP rows are full
 * and the tile form does not fit the register file (505 against 71 ms): not built.
 * The same holds for the pinned sweep of an M4Q_QP_EXACT_BOX solve (its time-batched tile form: config 3 exact 208 -> 190 ms).
 * M4Q_OPT_NO_TILE (or M4Q_NO_TILE=1 in the environment) keeps a session on the DPP sweeps (exact mode: the DPP pinned sweep for
 * general targets, which that kernel holds anyway).  M4Q_OPT_TILE is accepted and ignored (round 3's opt-in bit: the tile sweep is
 * no longer an option to ask for). */
#define M4Q_OPT_TILE 4
#define M4Q_OPT_NO_TILE 8
/* A traceless session whose per-member models were built by m4q_session_build_models from ONE set of generators and per-member
 * scales, with an order-1 library - member i's model is [I + dt s_i0 L_0 | dt s_i1 L_1 | ...] (vectorize.py:8-49 at order 1) -
 * runs the clipped solve on the shared generators wherever that form is built (d = 4): the workgroup holds one copy of dt L_k and per
 * member only I + dt s_i0 L_0, the other scales ride on the controls; 12.6 instead of 28.8 KB of LDS per workgroup, which lets d = 4
 * run two wavefronts per SIMD.  Same results to rounding (m4q_session_path: 4).  This bit (or M4Q_NO_SG=1 in the environment) keeps
 * such a session on its per-member models.  Uploaded models (m4q_session_upload) always do. */
#define M4Q_OPT_NO_SG 16

/* exit codes per instance (mpc.py:130,195,202,291): 0 normal, 1 exit_condition (set from the host with m4q_session_set_codes, or
 *   by the kernel itself for a condition given to m4q_session_set_exit),
 * 2 solver gave up (mpc.py:183-197 turns a cvxpy/OSQP warning into this; here: an M4Q_QP_EXACT_BOX solve that stopped at
 *   its iteration cap - the clipped Riccati solve cannot produce it), 3 non-finite objective (mpc.py:200-203; also where
 *   the reference would raise on NaN data: a batched engine cannot raise for one member).
 * A non-zero code ends that member's run at the step where it occurred: steps_done says how many steps are valid. */

typedef struct m4q_problem {
  int32_t dim_x;   /* n = d*d: 4, 9 or 16; also 8 (two reduced qubit states, experiment.py:238-306) with M4Q_PLANT_NONE;
                      n = d^4 = 16 with M4Q_PLANT_PROCESS */
  int32_t dim_u;   /* m */
  int32_t order;   /* control-library order (1 or 2; 1-4 for (16, 1): models of orders 3-4 are uploaded, m4q_session_build_models
                      and m4q_discretize_batch refuse them) */
  int32_t horizon; /* T (StepClock.horizon, mpc.py:17) */
  int32_t n_steps; /* StepClock.n_steps (mpc.py:18) */
  int32_t max_iter;   /* SQP iteration cap per MPC step (mpc.py:128, default 100) */
  int32_t warm_start; /* mpc.py:208 */
  int32_t qp_flags;
  int32_t plant_kind;
  int32_t model_per_instance;
  int32_t plant_per_instance;
  int32_t target_per_instance;
  int32_t target_cols; /* columns of X_targ; U_targ has the same count (extra ones unused) */
  int32_t reserved;    /* options: M4Q_OPT_FORCE_COMPLEX | M4Q_OPT_NO_TRACELESS | M4Q_OPT_TILE | M4Q_OPT_NO_TILE | M4Q_OPT_NO_SG */
  int32_t measure_freq; /* StepClock.measure_freq (mpc.py:19,252-267): the plant is measured every measure_freq-th step, the
                           model closes the loop in between; 0 or 1 = every step */
  int32_t reserved2;
  double dt;     /* StepClock.dt */
  double sat;    /* |u| <= sat (optimize.py:43, lqr.py:76) */
  double du;     /* first-control band (optimize.py:29-30); ignored without M4Q_QP_DU_BAND */
  double ls_tol; /* SQP stop: ||alpha dZ|| < ls_tol (mpc.py:224, 1e-4) */
} m4q_problem;

M4Q_API const char* m4q_last_error(void);
M4Q_API const char* m4q_version(void);
/* number of HIP devices visible; < 0 on error */
M4Q_API int m4q_device_count(void);
/* 1 if a kernel exists for this shape */
M4Q_API int m4q_supported(int32_t dim_x, int32_t dim_u, int32_t order);
/* number of non-constant monomials P for (order, dim_u) (linearize.size_of_library - 1) */
M4Q_API int m4q_library_size(int32_t order, int32_t dim_u);
/* exponent table in the reference's order, out[(P+1)*dim_u] (linearize.create_power_list) */
M4Q_API int m4q_power_list(int32_t order, int32_t dim_u, int32_t* out);

/* ---- fine-grained host entry points --------------------------------------------------------- */

/* replaces WrapModel.get_model_along_traj (linearize.py:61-70) for B trajectories.
 * models [B|1][n][n(1+P)] c, X [B][T][n] c (the T linearisation points), U [B][T][m] r
 * -> A_ls [B][T][n][n] c, B_ls [B][T][n][m] c, Delta_ls [B][T][n] c */
M4Q_API int m4q_linearize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t T, const double* models,
                        int32_t model_per_instance, const double* X, const double* U, double* A_ls, double* B_ls,
                        double* Delta_ls);

/* The PLANT's own discrete-time Jacobians along B trajectories, in one launch: where m4q_linearize_batch linearises a model (a
 * truncated discretisation, or a fit), this linearises the held-control step x+ = f(x, u) of the two unitary device plants
 * exactly, from U = expm(-i dts[t] (H0 + sum_k v_k H_k)) and its Frechet derivatives dU_k (one exponential of the (1 + m) d block
 * matrix, as the rollout gradients).  plant_linearize.py: plant_linearize_reference is the definition.
 * Member b at point t: state X[b][t], controls u = U[b|.][t], the member sees v_k = u_scale[b][k] u_k.
 *   A = (U (x) U^*) (x) I_cols (cols = 1: HAMILTONIAN, n = d^2; cols = d^2: PROCESS, n = d^4) - it does not depend on the state;
 *   B[:, k] = u_scale[b][k] vec(dU_k R U^H + U R dU_k^H), R = mat(x): the derivative with respect to the UNSCALED control u_k;
 *   Delta = -B u (summed with k ascending), so that A x + B u + Delta = f(x, u) to rounding (f(x, u) = A x holds exactly).
 * dts [T] r, X [B][T][n] c, U [B|1][T][m] r (u_per_instance), u_scale [B][m] r or NULL, op0 and ops as m4q_plant_rollout_batch
 * -> A_ls [B][T][n][n] c, B_ls [B][T][n][m] c, Delta_ls [B][T][n] c, the layouts of m4q_linearize_batch: they go into
 * m4q_quad_program_batch unchanged.  Each output may be NULL (A is 16 n^2 bytes per point and not always wanted), not all three.
 * M4Q_E_BADARG: B or T < 1 (or B T beyond 2^31 - 1); dts, X, U, op0 or ops missing; all outputs NULL; a plant_kind that is no device plant; M4Q_PLANT_PROCESS
 * on a dim_x that is no fourth power.  M4Q_E_UNSUPPORTED: no compiled shape; dim_x not a square; M4Q_PLANT_GENERATOR (no kernel:
 * linearise its discretised model, m4q_discretize_batch then m4q_linearize_batch).  All checked before a device is asked for. */
M4Q_API int m4q_plant_linearize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                              const double* X, const double* U, int32_t u_per_instance, const double* u_scale,
                              const double* op0, const double* ops, int32_t plant_per_instance,
                              double* A_ls, double* B_ls, double* Delta_ls);

/* replaces quad_program (optimize.py:12-60 statement; lqr.py:14-79 arithmetic) for B problems.
 * x_init [B][n] c, X_bm [B|1][T+1][n] c, U_bm [B|1][T][m] r, Q_ls [T+1][n][n] c, R_ls [T][m][m] c,
 * A_ls [B][T][n][n] c, B_ls [B][T][n][m] c, Delta_ls [B][T][n] c (NULL = zero),
 * u_prev [B][m] r (NULL = no band) -> X_opt [B][T+1][n] c, U_opt [B][T][m] r, cost [B] r,
 * gains [B][T][n+1][m] c (NULL to skip; gains[b][t][col][k] = Gains[t][k][col] of lqr.py:61).
 * With M4Q_QP_EXACT_BOX the gains are those of the final active-set iteration: a control that is free at the optimum has its
 * feedback row; a control PINNED on a bound at (t, k) has, in its slot, the affine form of its multiplier along the optimal
 * trajectory (row . (x_t - xbar_t) + const = dJ/du_tk, sign opposite to the side it is pinned on) - not the [0 | u - ubar] row
 * a constant control would have. */
M4Q_API int m4q_quad_program_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t T, int32_t qp_flags, double sat, double du,
                           const double* x_init, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                           const double* Q_ls, const double* R_ls, const double* A_ls, const double* B_ls,
                           const double* Delta_ls, const double* u_prev, double* X_opt, double* U_opt, double* cost,
                           double* gains);

/* The QP of m4q_quad_program_batch posed on the linearisation m4q_plant_linearize_batch would return along each member's own
 * nominal trajectory, in ONE call: A_ls, B_ls and Delta_ls never exist on the host.  Two launches on one stream: the first leaves
 * the d x d propagator U_t (A_t = (U_t (x) U_t^*) (x) I_cols is formed from it where it is used: 16 d^2 bytes per point instead
 * of 16 n^2), B_t and Delta_t in device workspaces, the second is the Riccati sweep and rollout of m4q_quad_program_batch over
 * them.  plant_linearize.py: plant_quad_program_reference is the definition.
 * The plant side as m4q_plant_linearize_batch: dts [T] r, X [B][T][n] c (the linearisation points), U [B|1][T][m] r
 * (u_per_instance), u_scale [B][m] r or NULL, op0, ops, plant_per_instance.  The QP side as m4q_quad_program_batch: qp_flags, sat,
 * du, x_init [B][n] c (NULL: X[b][0]), X_bm, U_bm, bm_per_instance, Q_ls, R_ls, u_prev [B][m] r or NULL
 * -> X_opt [B][T+1][n] c, U_opt [B][T][m] r, cost [B] r, gains [B][T][n+1][m] c (NULL to skip).  M4Q_QP_EXACT_BOX as there: the same
 * workspace and 4 GiB limit, the same meaning of the gains.
 * M4Q_E_BADARG: B or T < 1 (or B T beyond 2^31 - 1); a required array missing; sat not positive; qp_flags that
 * m4q_quad_program_batch refuses; a plant_kind that is no device plant; M4Q_PLANT_PROCESS on a dim_x that is no fourth power.
 * M4Q_E_UNSUPPORTED: no compiled shape; dim_x not a square; a plant-only shape (no QP kernel); M4Q_PLANT_GENERATOR (no kernel:
 * m4q_discretize_batch + m4q_linearize_batch + m4q_quad_program_batch).  All checked before a device is asked for. */
M4Q_API int m4q_plant_quad_program_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                                 const double* X, const double* U, int32_t u_per_instance, const double* u_scale,
                                 const double* op0, const double* ops, int32_t plant_per_instance,
                                 int32_t qp_flags, double sat, double du, const double* x_init, const double* X_bm,
                                 const double* U_bm, int32_t bm_per_instance, const double* Q_ls, const double* R_ls,
                                 const double* u_prev, double* X_opt, double* U_opt, double* cost, double* gains);

/* Controls optimised on the plant itself: a Gauss-Newton SQP for B members in ONE call.  Each iteration is the QP of
 * m4q_plant_quad_program_batch on the plant's Jacobians along the member's current trajectory, then a line search on the TRUE plant
 * over the `steps` candidates clip(U + 2^-j (U_opt - U)), j = 0 .. steps-1: the smallest j attaining the least cost wins, is accepted
 * if that cost is below the current one, and the member stops as converged when the decrease is at most tol times the cost.  The
 * plant, the targets, the weights, x0 and U0 are staged once; the iterate and the workspaces stay on the device and the launches
 * follow one another on one stream without a host synchronisation.  plant_sqp.py: plant_sqp_reference is the definition.
 * The plant side as m4q_plant_quad_program_batch, with x0 [B][n] c and the first guess U0 [B|1][T][m] r (u_per_instance; clipped into
 * the bounds) in place of X, U and x_init; the QP side as there; iters in 1..64, steps in 1..8, tol >= 0
 * -> X [B][T+1][n] c, U [B][T][m] r, cost [B] r, cost_hist [B][iters+1] r (entry 0: the first guess; unused entries repeat the last
 * cost), alpha_hist [B][iters] r (the accepted step lengths; unused entries 0), n_iter [B], status [B] (0 iterations used up,
 * 1 converged, 2 no candidate lowered the cost: U, X and cost are kept, 3 the first cost was not finite), gains [B][T][n+1][m] c
 * (NULL to skip): the QP's at the returned (X, U), whatever the status.
 * M4Q_E_BADARG, M4Q_E_UNSUPPORTED: what m4q_plant_quad_program_batch refuses; iters, steps or tol outside their ranges; x0 or U0
 * missing.  All checked before a device is asked for. */
M4Q_API int m4q_plant_sqp_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                        const double* x0, const double* U0, int32_t u_per_instance, const double* u_scale,
                        const double* op0, const double* ops, int32_t plant_per_instance,
                        int32_t qp_flags, double sat, double du, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                        const double* Q_ls, const double* R_ls, const double* u_prev, int32_t iters, int32_t steps, double tol,
                        double* X, double* U, double* cost, double* cost_hist, double* alpha_hist, int32_t* n_iter, int32_t* status,
                        double* gains);

/* m4q_plant_sqp_batch with a CLOSED-LOOP line search: an iLQR on the plant itself for B members in ONE call.  The loop, the
 * statuses, the histories, the tol rule and the tie rule are m4q_plant_sqp_batch's; only the candidates differ.  Candidate j,
 * a = 2^-j, runs the QP's law on the true plant around the iterate (Xbar, Ubar): from x_0 = x0, for a control the QP leaves free
 *     u_t = clip(Ubar_t + a (Re(K_t (Xbar_t - xb_t)) + Re(k_t) + ub_t - Ubar_t) + Re(K_t (x_t - Xbar_t)))
 * with [K_t; k_t] the gains of this iteration's QP, and for a control M4Q_QP_EXACT_BOX left on a bound (its slot of the gains holds
 * a multiplier row) u_t = clip(Ubar_t + a (U_opt_t - Ubar_t)).  At a = 1 a free control is the stored law of
 * m4q_plant_feedback_batch on the plant; as a -> 0 the candidate is the iterate.  The gains never leave the device between the QP
 * and the forward pass.  plant_ilqr.py: plant_ilqr_reference is the definition.
 * Arguments, outputs and refusals: those of m4q_plant_sqp_batch, in its order.  All checked before a device is asked for. */
M4Q_API int m4q_plant_ilqr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t T, const double* dts,
                         const double* x0, const double* U0, int32_t u_per_instance, const double* u_scale,
                         const double* op0, const double* ops, int32_t plant_per_instance,
                         int32_t qp_flags, double sat, double du, const double* X_bm, const double* U_bm, int32_t bm_per_instance,
                         const double* Q_ls, const double* R_ls, const double* u_prev, int32_t iters, int32_t steps, double tol,
                         double* X, double* U, double* cost, double* cost_hist, double* alpha_hist, int32_t* n_iter, int32_t* status,
                         double* gains);

/* replaces vectorize.discretize_homogeneous (vectorize.py:8-49) for B operator sets: the Taylor/Dyson expansion of
 * exp(dt (G_0 + sum_k u_k G_k)) to `order`, binned by control monomial.
 * generators [B|1][1+m][n][n] c, scaled per member by scales [B][1+m] r when given (NULL = 1) -> models [B][n][n(1+P)] c */
M4Q_API int m4q_discretize_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, double dt, const double* generators,
                         int32_t gen_per_instance, const double* scales, double* models);

/* replaces QExperiment.simulate over one held-control step (experiment.py:202-212, mpc.py:256-260).
 * x [B][n] c, u [B][m] r, op0 [B|1][k][k] c, ops [B|1][m][k][k] c with k = d (HAMILTONIAN, n = d^2), n (GENERATOR) or
 * d (PROCESS, n = d^4)
 * -> x_next [B][n] c */
M4Q_API int m4q_plant_step_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, double dt, const double* x,
                         const double* u, const double* op0, const double* ops, int32_t plant_per_instance,
                         double* x_next);

/* Open-loop rollouts: a known control sequence applied to B members over N steps in ONE launch (QExperiment.simulate /
 * DMDc.predict along a sequence, for an ensemble).  The state stays in registers from x0 to the last step.
 * x0 [B][n] c; u [B|1][N][m] r (u_per_instance 0: one sequence shared by the ensemble); u_scale [B][m] r or NULL: member b sees
 * u_scale[b][k] u[t][k], formed on the device in fp64.
 * Outputs, each optional: xs_mode 0 none, 1 the final state xs [B][n] c, 2 the whole trajectory xs [B][N+1][n] c (column 0 = x0 as
 * given); q_mode 0 / 1 / 2 likewise the figure q = Re((x - f)^H W (x - f)) as q [B] or [B][N+1] r, with W [n][n] c shared and
 * target f [B|1][n] c (both NULL when q_mode is 0).
 * M4Q_E_BADARG: B or N < 1, a missing required array, a mode outside 0-2, both modes 0, q_mode != 0 without W or target, (plant) a
 * plant_kind that is no device plant, M4Q_PLANT_PROCESS with n not a fourth power.  M4Q_E_UNSUPPORTED: no compiled shape, a plant
 * rollout with n not a square, a model rollout on a plant-only shape.  Arguments are checked before the device is asked for.
 *
 * m4q_plant_rollout_batch: step t is the held-control step of m4q_plant_step_batch over dts[t] (dts [N] r: a non-uniform time grid
 * works); op0 / ops as there. */
M4Q_API int m4q_plant_rollout_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                            const double* x0, const double* u, int32_t u_per_instance, const double* u_scale, const double* op0,
                            const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                            int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q);
/* m4q_model_rollout_batch: step t is x+ = A [x ; lift_u(u_t) (x) x] (model.py:81-93), what the closed loop applies on a step it does
 * not measure; models [B|1][n][n(1+P)] c.  Complex arithmetic whatever the model. */
M4Q_API int m4q_model_rollout_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* u,
                            int32_t u_per_instance, const double* u_scale, const double* models, int32_t model_per_instance,
                            const double* W, const double* target, int32_t target_per_instance, int32_t xs_mode, double* xs,
                            int32_t q_mode, double* q);

/* Control gradients of the open-loop rollouts, for B members in ONE launch: what polishing a pulse against an ensemble (robust GRAPE)
 * needs.  mpc4quantum_amd/grad.py (plant_rollout_grad_reference, model_rollout_grad_reference, ordered_weighted_sum) is the
 * definition, in NumPy and SciPy, in the kernels' order of operations.
 * The arguments up to target_per_instance are the rollouts' own.  Member b sees v[t][k] = u_scale[b][k] u[t][k]; with d_t = x_t - f and
 * q_t = Re(d_t^H W d_t) (W need not be Hermitian) the objective is J = q_N (q_mode 1) or J = sum_{t=0..N} q_t (q_mode 2).
 * -> q [B] (q_mode 1) or [B][N+1] (q_mode 2) r, required: the forward pass is the rollouts' own step, so q equals their figure bit
 *    for bit; grad [B][N][m] r, required: dJ_b/du[t][k], the derivative with respect to the unscaled sequence the caller passed;
 *    grad_scale [B][m] r or NULL: dJ_b/du_scale[b][k] = sum_t u[t][k] dJ_b/dv[t][k], t ascending.
 * reduce != 0 (only with u_per_instance 0): grad is [N][m] = sum_b w_b grad[b][t][k] and q_mean [1] = sum_b w_b J_b (required), with
 * w = weights [B] r (finite, non-negative) or, weights NULL, 1/B.  The order is fixed: members in ascending chunks of 256, a
 * sequential sum inside a chunk, then a sequential sum of the chunk partials; every product w_b g is rounded before it is added.
 * The members' gradients then stay on the device: [N][m], q_mean and q are all that is copied back.  Without reduce, weights
 * are checked and otherwise unused.
 * The adjoint pass keeps the forward states in a device workspace [B][N+1][n] c, allocated by the call, and recomputes each step's
 * propagator with its Frechet derivatives from one matrix exponential of the (1 + m) d block matrix (every compiled plant shape
 * keeps (1 + m) d <= 16).
 * M4Q_E_BADARG: B or N < 1, a missing x0, u, W, target, q or grad, q_mode outside 1-2, reduce with u_per_instance 1 or without
 * q_mean, a non-finite or negative weight, (plant) missing dts, op0 or ops, a plant_kind that is no device plant,
 * M4Q_PLANT_PROCESS with n not a fourth power.  M4Q_E_UNSUPPORTED: no compiled shape, a plant gradient with n not a square, a
 * model gradient on a plant-only shape, and M4Q_PLANT_GENERATOR: its block matrix has (1 + m) n > 16 columns - dissipative
 * dynamics go through the gradient of the discretised model (m4q_discretize_batch, then m4q_model_rollout_grad_batch).
 * Arguments are checked before the device is asked for.
 *
 * m4q_plant_rollout_grad_batch: M4Q_PLANT_HAMILTONIAN (n = d^2) and M4Q_PLANT_PROCESS (n = d^4); dts, op0, ops as
 * m4q_plant_rollout_batch. */
M4Q_API int m4q_plant_rollout_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                 const double* x0, const double* u, int32_t u_per_instance, const double* u_scale, const double* op0,
                                 const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                                 int32_t target_per_instance, int32_t q_mode, const double* weights, int32_t reduce, double* q,
                                 double* grad, double* grad_scale, double* q_mean);
/* m4q_model_rollout_grad_batch: the step of m4q_model_rollout_batch; models [B|1][n][n(1+P)] c. */
M4Q_API int m4q_model_rollout_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0,
                                 const double* u, int32_t u_per_instance, const double* u_scale, const double* models,
                                 int32_t model_per_instance, const double* W, const double* target, int32_t target_per_instance,
                                 int32_t q_mode, const double* weights, int32_t reduce, double* q, double* grad, double* grad_scale,
                                 double* q_mean);

/* Plant-parameter gradient of an open-loop plant rollout against a measured trajectory, for B members in ONE launch: what fitting
 * detunings, anharmonicities, crosstalk strengths and drive gains to data needs.  mpc4quantum_amd/plant_param.py
 * (plant_param_grad_reference) is the definition.
 * The arguments up to plant_per_instance are m4q_plant_rollout_batch's.  dirs [B|1][p][d][d] c: Hermitian directions D_j; member b's
 * drift is understood as op0_b + sum_j theta_j D_j, evaluated at the op0_b passed in.  data [B|1][N+1][n] c: the trajectory y the
 * rollout is compared with; col_w [N+1] r (finite, non-negative) or NULL (ones): a column whose weight is 0 is skipped (sparse
 * measurement), the costate still propagates through it.  W [n][n] c need not be Hermitian.
 * -> J [B] r, required: J_b = sum_t col_w[t] Re((x_t - y_t)^H W (x_t - y_t)), t ascending from 0.0, each figure the one
 *    m4q_plant_rollout_batch returns for that column;
 *    grad_theta [B][p] r, required: dJ_b/dtheta_j;
 *    grad_scale [B][m] r or NULL: dJ_b/du_scale[b][k] of the same objective.
 * One matrix exponential of the (1 + p_tot) d block matrix per step gives the propagator and its Frechet derivatives in all
 * p_tot = p + (grad_scale ? m : 0) directions; the block must fit the 16 lanes of a row: p_tot <= 16 / d - 1 (7 at d = 2, 4 at
 * d = 3, 3 at d = 4).  The forward states stay in a device workspace [B][N+1][n] c, allocated by the call.
 * M4Q_E_BADARG: B, N or p < 1, a missing x0, u, W, data, dts, op0, ops, dirs, J or grad_theta, a col_w entry that is not finite or
 * negative, a plant_kind that is no device plant (M4Q_PLANT_NONE included), M4Q_PLANT_PROCESS with n not a fourth power.
 * M4Q_E_UNSUPPORTED: no compiled shape, n not a square, a plant-only shape (the kernels are built with the auxiliary ones),
 * M4Q_PLANT_GENERATOR, and more directions than the shape allows (the message names the limit).
 * Arguments are checked before the device is asked for. */
M4Q_API int m4q_plant_rollout_param_grad_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                       const double* x0, const double* u, int32_t u_per_instance, const double* u_scale,
                                       const double* op0, const double* ops, int32_t plant_per_instance, int32_t p, const double* dirs,
                                       int32_t dirs_per_instance, const double* W, const double* data, int32_t data_per_instance,
                                       const double* col_w, double* J, double* grad_theta, double* grad_scale);

/* S control sequences, each SHARED by the ensemble, rolled against all B members in ONE launch: compare pulses or scan an amplitude
 * over an ensemble; the line search of m4q_plant_robust_batch.  us [S][N][m] r, 1 <= S <= 8; the other arguments up to q_mode as
 * m4q_plant_rollout_grad_batch with u_per_instance 0.  No state is stored.
 * -> J [B][S] r or NULL: member b's objective under us[s], q_N (q_mode 1) or sum_{t=0..N} q_t with t ascending from 0.0 (q_mode 2);
 *    J[.][s] has the bits of m4q_plant_rollout_batch's figure under us[s] (q_mode 2: of its N + 1 columns added in that order).
 *    F [S] r or NULL: sum_b w_b J[b][s] in the gradient's fixed order, w = weights [B] r (finite, non-negative) or, NULL, 1/B.
 * M4Q_E_BADARG: the gradient's refusals, S outside 1-8, q_mode outside 1-2, J and F both NULL.  M4Q_E_UNSUPPORTED: no compiled
 * shape, n not a square, and M4Q_PLANT_GENERATOR (its kernels live in the other object; roll its discretised model).
 * Arguments are checked before the device is asked for. */
M4Q_API int m4q_plant_rollout_multi_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                  const double* x0, int32_t S, const double* us, const double* u_scale, const double* op0,
                                  const double* ops, int32_t plant_per_instance, const double* W, const double* target,
                                  int32_t target_per_instance, int32_t q_mode, const double* weights, double* J, double* F);

/* ONE control sequence optimised against the weighted mean of an ensemble (robust GRAPE) in one call: a projected L-BFGS on
 * F(U) = sum_b w_b J_b(U), |U[t][k]| <= sat.  mpc4quantum_amd/plant_robust.py is the definition (its docstring states the loop step
 * by step); csrc/m4q_robust_host.h repeats its direction in the same order of operations.
 * The ensemble - plant, x0, u_scale, W, targets, weights, dts - is staged ONCE, with the gradient's state workspace [B][N+1][n] c.
 * An iteration is one launch of the reduced gradient (m4q_plant_rollout_grad_batch with reduce) at the iterate and one launch of
 * m4q_plant_rollout_multi_batch's kernel on the `steps` candidates clip(U + 2^-j p); the direction p and the decision are taken on
 * the host in between: [N][m] + 1 doubles come down, [steps][N][m] go up, `steps` doubles come down.  The ensemble and its states
 * never leave the device.  The gradient is not taken again when U did not move.
 * U0 [N][m] r: the first guess (clipped into the box).  sat > 0 (INFINITY: no box); iters in 1..64; steps in 1..8; mem in 0..8
 * pairs of quasi-Newton memory (0: projected gradient); step0 > 0 finite: the largest entry of the first trial step of a
 * memoryless direction; tol, gtol >= 0 finite: stop when F - F_new <= tol |F| or max |projected gradient| <= gtol.
 * -> U [N][m] r, cost [1], cost_hist [iters+1] (entry 0 the first F; unused entries repeat the last cost), alpha_hist [iters] (the
 *    accepted 2^-j; 0: rejected or unused), pgrad_hist [iters] (max |projected gradient|; unused 0), n_iter [1] (iterations begun),
 *    status [1]: 0 iterations used up, 1 converged, 2 no descent, 3 the first cost was not finite.
 *    J [B] r or NULL: the members' objectives at U, by one more launch with S = 1 (whose F equals cost bit for bit).
 * Refusals: those of m4q_plant_rollout_grad_batch with reduce, and the ranges above (M4Q_E_BADARG); M4Q_PLANT_GENERATOR is
 * M4Q_E_UNSUPPORTED: optimise on the discretised model's gradient.  All checked before a device is asked for. */
M4Q_API int m4q_plant_robust_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                                  const double* x0, const double* U0, const double* u_scale, const double* op0, const double* ops,
                                  int32_t plant_per_instance, const double* W, const double* target, int32_t target_per_instance,
                                  int32_t q_mode, const double* weights, double sat, int32_t iters, int32_t steps, int32_t mem,
                                  double step0, double tol, double gtol, double* U, double* cost, double* cost_hist,
                                  double* alpha_hist, double* pgrad_hist, int32_t* n_iter, int32_t* status, double* J);

/* The model twins of the two calls above: the same multi rollout and the same optimiser on the members' MODELS
 * (models [B|1][n][n(1+P)] c, the step of m4q_model_rollout_batch) - dissipative dynamics through their discretised generators
 * (m4q_discretize_batch), identified models (m4q_dmdc_fit_batch), any shape with a model kernel.  mpc4quantum_amd/model_robust.py
 * is the definition: plant_robust.py's loop on model_rollout_grad_reference(reduce) and model_rollout_multi_reference.
 * m4q_model_rollout_multi_batch: J[.][s] has the bits of m4q_model_rollout_batch's figure under us[s] (q_mode 2: of its N + 1
 * columns added with t ascending from 0.0); F as above.  The member's model is staged once per launch, not once per sequence.
 * m4q_model_robust_batch: m4q_plant_robust_batch's loop, step for step, on m4q_model_rollout_grad_batch with reduce and the multi
 * rollout's kernel; the ensemble - models, x0, u_scale, W, targets, weights - and every workspace are staged once.
 * Refusals: those of m4q_model_rollout_grad_batch with reduce (M4Q_E_UNSUPPORTED: no model kernel for (dim_x, dim_u, order);
 * M4Q_E_BADARG: B or N < 1, a missing x0, sequence, W, target or models, q_mode outside 1-2, a non-finite or negative weight), then
 * the ranges of the plant twins (S, iters, steps, mem, sat, step0, tol, gtol, the required outputs; J and F both NULL).  All
 * checked before a device is asked for, under the entry's name. */
M4Q_API int m4q_model_rollout_multi_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, int32_t S,
                                  const double* us, const double* u_scale, const double* models, int32_t model_per_instance,
                                  const double* W, const double* target, int32_t target_per_instance, int32_t q_mode,
                                  const double* weights, double* J, double* F);
M4Q_API int m4q_model_robust_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0, const double* U0,
                                  const double* u_scale, const double* models, int32_t model_per_instance, const double* W,
                                  const double* target, int32_t target_per_instance, int32_t q_mode, const double* weights,
                                  double sat, int32_t iters, int32_t steps, int32_t mem, double step0, double tol, double gtol,
                                  double* U, double* cost, double* cost_hist, double* alpha_hist, double* pgrad_hist, int32_t* n_iter,
                                  int32_t* status, double* J);

/* A stored feedback law run on B members over N steps in ONE launch: the tier between the open-loop rollouts above and the closed
 * loop that re-solves a QP at every step - time-varying gains around a nominal trajectory with saturation, a slew band and
 * measurement noise.  mpc4quantum_amd/feedback.py (FeedbackLaw, plant_feedback_reference, model_feedback_reference) is the
 * definition, in NumPy and SciPy.
 * The law: gains [B|1][N][n+1][m] c, the layout m4q_quad_program_batch returns (gains[t][col][k], col = n the affine column),
 * x_ref [B|1][N][n] c, u_ref [B|1][N][m] r - all three per member or all three shared (law_per_instance).  Step t of member b in
 * state x_t:
 *   s_k = sum_j Re(K_t[j][k] (x_t - x_ref[t])_j) + Re(K_t[n][k]) + u_ref[t][k];   lo = -sat, hi = sat (sat > 0, INFINITY: no box);
 *   du_band != 0: lo = fmax(lo, p_k - du), hi = fmin(hi, p_k + du) with p = u_prev[b] ([B|1][m] r) at t = 0, then u_{t-1};
 *   u_t[k] = fmin(fmax(s_k, lo), hi) (lo > hi: hi wins);   x_{t+1} = step(x_t, u_scale[b] u_t);
 *   noise_mode != 0: x_{t+1} += the draw of (seed, member_base + b, t + 1, component) scaled by sigma [B|1] r, as
 *   m4q_noise_sample_batch returns it - the noisy state is stored, read by the next control and stepped from; x0 is never measured.
 * x0, u_scale, W, target, xs_mode, xs, q_mode, q as the rollouts (column 0 of xs = x0 as given).  Further outputs:
 * us [B][N][m] r or NULL: the commanded u_t, before u_scale; clipped [B] i32 or NULL: the number of (t, k) with s_k <= lo or
 * s_k >= hi; status [B] i32, required: 0, or 3 when a state or a control of the member was not finite.
 * M4Q_E_BADARG: B or N < 1, a missing x0, gains, x_ref, u_ref or status, sat <= 0 or NaN, du_band with du <= 0 or not finite or
 * without u_prev, a mode outside 0-2, xs_mode and q_mode 0 with neither us nor clipped, a mode without its array, q_mode != 0
 * without W or target, a noise mode outside 0-2 or without sigma (or a sigma that is negative or not finite), M4Q_NOISE_HERMITIAN
 * on M4Q_PLANT_PROCESS or with n not a square, (plant) missing dts, op0 or ops, a plant_kind that is no device plant,
 * M4Q_PLANT_PROCESS with n not a fourth power.  M4Q_E_UNSUPPORTED: the cases of the rollouts.  Arguments are checked before the
 * device is asked for.
 *
 * m4q_plant_feedback_batch: the step of m4q_plant_rollout_batch (dts, op0, ops, plant_kind as there; all three device plants). */
M4Q_API int m4q_plant_feedback_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t plant_kind, int32_t N, const double* dts,
                             const double* x0, const double* gains, const double* x_ref, const double* u_ref,
                             int32_t law_per_instance, double sat, int32_t du_band, double du, const double* u_prev,
                             int32_t u_prev_per_instance, const double* u_scale, const double* op0, const double* ops,
                             int32_t plant_per_instance, int32_t noise_mode, const double* sigma, int32_t sigma_per_instance,
                             uint64_t seed, uint64_t member_base, const double* W, const double* target,
                             int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q, double* us,
                             int32_t* clipped, int32_t* status);
/* m4q_model_feedback_batch: the step of m4q_model_rollout_batch; models [B|1][n][n(1+P)] c. */
M4Q_API int m4q_model_feedback_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t N, const double* x0,
                             const double* gains, const double* x_ref, const double* u_ref, int32_t law_per_instance, double sat,
                             int32_t du_band, double du, const double* u_prev, int32_t u_prev_per_instance, const double* u_scale,
                             const double* models, int32_t model_per_instance, int32_t noise_mode, const double* sigma,
                             int32_t sigma_per_instance, uint64_t seed, uint64_t member_base, const double* W, const double* target,
                             int32_t target_per_instance, int32_t xs_mode, double* xs, int32_t q_mode, double* q, double* us,
                             int32_t* clipped, int32_t* status);

/* DMDc identification for an ensemble in ONE launch: DiscrepDMDc.from_data(X2, X1, krtimes(lift(U1), X1), rcond) = X2 pinv(Z, rcond)
 * (model.py: DiscrepDMDc.from_data, the fit of the reference's training workflow) for B members and R cut-offs, the models in the layout every other
 * entry point takes.  mpc4quantum_amd/fit.py (dmdc_fit_reference) is the definition, in NumPy, in the kernel's order of operations.
 * Member b has E experiments of N steps: xs [B][E][N+1][n] c, u [B|1][E][N][m] r (u_per_instance 0: one set shared by the ensemble),
 * u_scale [B][m] r or NULL: the member saw u_scale[b][k] u[e][t][k], formed on the device in fp64 as the rollouts form it.
 * Every snapshot (e, t) gives z = [x_t ; lift(u_t) (x) x_t] (the monomials of m4q_power_list without the constant, Kronecker row
 * p n + j; nz = n (1 + P)).  G = sum z z^H and C = sum x_{t+1} z^H are accumulated (e outer, t inner), G = V diag(lam) V^H comes from
 * cyclic-by-rows Jacobi with complex Hermitian rotations (a rotation is skipped when |g_pq| <= eps sqrt(g_pp g_qq), the iteration
 * stops after a sweep without rotations, 30 sweeps at the most), and for each rconds[r] the eigenpairs with
 * lam > rconds[r]^2 max(lam) give A_r = C V_k diag(lam_k)^-1 V_k^H: numpy's pinv cuts the singular values s = sqrt(lam) at
 * s > rcond max(s).  The decomposition is done once; every cut-off costs one truncated product.
 * rconds [R], 1 <= R <= M4Q_FIT_MAX_RCONDS, each in [M4Q_FIT_RCOND_MIN, 1) = [1e-7, 1): below that the cut-off rcond^2 lies in the
 * Gram matrix's own rounding floor (~ nz eps) and the rank cannot be decided from G - fit with rcond = 1e-15 on the host
 * (DiscrepDMDc.from_data, an SVD of the data themselves).
 * -> models [R][B][n][n(1+P)] c; ranks [R][B] (the eigenpairs kept) or NULL; svals [B][nz] r or NULL: the singular values of the
 * stacked data, descending, s_k = sqrt(sum |v_k^H z|^2) - lam_k = v_k^H G v_k taken from the snapshots themselves in a second pass
 * over them, so a vanishing singular value comes back at ~eps s_0 and not at sqrt of G's rounding floor; status [B]: 0 ok, 1 the Jacobi iteration hit its cap (the models are written from
 * the last iterate), 3 non-finite data (zero models and singular values, rank 0).
 * M4Q_E_BADARG: B, E, N or R < 1, R > 16, an rcond outside the range (or NaN), a missing xs, u, rconds, models or status.
 * M4Q_E_UNSUPPORTED: no compiled shape, a plant-only shape, a shape whose LDS layout (2 nz^2 + n nz complex numbers) exceeds one
 * workgroup's 160 KiB - (16, 1, 4), nz = 80.  Arguments are checked before the device is asked for. */
#define M4Q_FIT_MAX_RCONDS 16
#define M4Q_FIT_RCOND_MIN 1e-7
M4Q_API int m4q_dmdc_fit_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                       const double* u, int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R,
                       double* models, int32_t* ranks, double* svals, int32_t* status);

/* The same fit, same arguments and results, from a QR of the data themselves and not from their Gram matrix: the error of A is
 * O(eps kappa) where m4q_dmdc_fit_batch's is O(eps kappa^2), and ranks are decided down to rcond = 1e-12.  Prefer it when the data
 * are ill-conditioned (noise-free trajectories, cut-offs at the low end of the training grid) or rcond < 1e-7 is wanted;
 * m4q_dmdc_fit_batch is the cheaper one.  mpc4quantum_amd/fit.py (dmdc_fit_qr_reference) is the definition, in NumPy, in the
 * kernel's order of operations.  Per member:
 * - every snapshot (e outer, t inner) contributes the row (z^H | x_{t+1}^H), rotated into R [nz][nz] (upper triangular, from 0) and
 *   T [nz][n] (from 0) by Givens rotations j = 0 .. nz-1: with a = R[j][j], b = row[j] (skipped when b = 0),
 *   h = sqrt(|a|^2 + |b|^2), c = a / h, s = b / h: R[j][j:] <- conj(c) R[j][j:] + conj(s) row[j:], row[j:] <- c row[j:] - s R[j][j:],
 *   the same on T[j] and the right-hand side.  Then Z^H = Q R and T = Q^H Y^H.
 * - one-sided (Hestenes) Jacobi on the columns of M = R, V = I accumulated, pairs cyclic by rows: with a_pp = m_p^H m_p,
 *   a_qq = m_q^H m_q, g = m_p^H m_q the rotation and the skip rule (|g| <= eps sqrt(a_pp a_qq)) of m4q_dmdc_fit_batch; the iteration
 *   stops after a sweep without rotations, 30 sweeps at the most.
 * - lam_k = m_k^H m_k; svals = sqrt(lam) descending (no second pass over the data); for each rconds[r] the k with
 *   lam_k > rconds[r]^2 max(lam) give A_r = sum_k (T^H m_k / lam_k) v_k^H.
 * rconds each in [M4Q_FIT_QR_RCOND_MIN, 1) = [1e-12, 1): the singular values come out to a few eps s_0, so a cut-off a factor 1.2
 * from every singular value is decidable down to about 1e3 eps; numpy's default 1e-15 lies inside the rounding of the data
 * themselves and stays a host call (DiscrepDMDc.from_data).
 * status [B]: 0 ok, 1 the Jacobi iteration hit its cap (the models are written from the last iterate), 3 non-finite data (R or T
 * holds a non-finite entry: zero models and singular values, rank 0).
 * M4Q_E_BADARG and M4Q_E_UNSUPPORTED: the argument classes of m4q_dmdc_fit_batch, with this entry point's rcond range (R, V and T
 * take the room of G, V and C, so the same shapes fit).  Arguments are checked before the device is asked for. */
#define M4Q_FIT_QR_RCOND_MIN 1e-12
M4Q_API int m4q_dmdc_fit_qr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                          const double* u, int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R,
                          double* models, int32_t* ranks, double* svals, int32_t* status);

/* The two fits against a prior model: one DiscrepDMDc.fit_iteration (model.py:186-207) for B members in ONE launch,
 *   A_r = A0 + (Y - A0 Z) pinv(Z, rconds[r]) on the discounted stacks = A0 (I - Pi_r) + Y Z_r^+,
 * the fit where the data excited the plant, the prior A0 everywhere else.  m4q_dmdc_refit_batch takes m4q_dmdc_fit_batch's route,
 * m4q_dmdc_refit_qr_batch m4q_dmdc_fit_qr_batch's; the first 16 arguments, the results and the rcond range are that entry point's.
 * mpc4quantum_amd/fit.py (dmdc_fit_reference / dmdc_fit_qr_reference with A0, discount, counts) is the definition.
 * A0 [B|1][n][nz] c: the prior model (A0_per_instance 0: one for the ensemble); discount [B|1] r, each in (0, 1]: snapshot s of the S
 * a member takes has weight discount^(S-1-s); counts [B] or NULL: member b takes only t < counts[b] of every experiment
 * (0 <= counts[b] <= N), as m4q_online_dmdc_batch does.  Per member:
 * - Gram route: before a snapshot is accumulated G <- d2 G, C <- d2 C (and the sums behind svals likewise), d2 = discount * discount
 *   formed once and each product rounded on its own; after the last one D[i][l] = C[i][l] - sum_k A0[i][k] G[k][l] (k ascending, the
 *   terms subtracted one at a time) takes C's place.
 * - QR route: R <- discount R, T <- discount T before a snapshot's rotations; after the last one
 *   T[j][i] <- T[j][i] - sum_{k >= j} R[j][k] conj(A0[i][k]), k ascending.
 * - spectrum, ranks, svals (those of the weighted stack) and truncated products as in the plain fit; A0 is added once to every entry
 *   of every A_r.  With A0 = 0, discount = 1 and counts NULL (or N) the results are the plain fit's, number for number.
 * status [B]: as the plain fit, and 3 also for a non-finite A0 (zero models).  counts[b] = 0: models = A0, rank 0, status 0.
 * M4Q_E_BADARG: what the plain fit refuses, a missing A0 or discount, a discount outside (0, 1] (or NaN), a count outside [0, N].
 * M4Q_E_UNSUPPORTED: exactly where the plain fit returns it.  Arguments are checked before the device is asked for. */
M4Q_API int m4q_dmdc_refit_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                         const double* u, int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R,
                         double* models, int32_t* ranks, double* svals, int32_t* status, const double* A0,
                         int32_t A0_per_instance, const double* discount, int32_t discount_per_instance, const int32_t* counts);
M4Q_API int m4q_dmdc_refit_qr_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                         const double* u, int32_t u_per_instance, const double* u_scale, const double* rconds, int32_t R,
                         double* models, int32_t* ranks, double* svals, int32_t* status, const double* A0,
                         int32_t A0_per_instance, const double* discount, int32_t discount_per_instance, const int32_t* counts);

/* Recursive DMDc updates for an ensemble in ONE launch: OnlineDMDc.fit_iteration (model.py:216-313, recursive least squares with a
 * forgetting factor) fed with every snapshot of B members - what mpc(..., streaming=True) does to its model, for an ensemble.
 * mpc4quantum_amd/online.py (online_dmdc_reference) is the definition, in NumPy, in the kernel's order of operations.
 * The snapshots are m4q_dmdc_fit_batch's: xs [B][E][N+1][n] c, u [B|1][E][N][m] r, u_scale [B][m] r or NULL, z = [x_t ; lift(u_t) (x) x_t],
 * y = x_{t+1}, e outer, t inner; counts [B] or NULL: member b takes only t < counts[b] of every experiment (0 <= counts[b] <= N).
 * State: A [n][nz] from A0 [B|1][n][nz] c, P [nz][nz] from P0 [B|1][nz][nz] c or, with P0 NULL, alpha I (alpha > 0);
 * discount [B|1] r, each in (0, 1].  One update, sums in ascending index:
 *   Pz = P z;  w = Pz (M4Q_ONLINE_HERMITIAN: w_j = sum_i conj(z_i) P[i][j]);  gamma = 1 / (1 + sum_j w_j z_j);  r = y - A z;
 *   A[i][j] += (gamma r_i) w_j;  P[i][j] = (P[i][j] - (gamma Pz_i) w_j) * (1 / discount), the reciprocal formed once per member.
 * -> models [B][n][nz] c (the layout every other entry point takes); P [B][nz][nz] c or NULL; hist [E N / hist_every][B][n][nz] c
 * or NULL: A after updates hist_every, 2 hist_every, ... (written only when hist_every > 0; records a member does not reach are
 * zero); innov [B][E N] r or NULL: sum_i |r_i|^2 of each snapshot before its update, at e N + t (zero beyond counts);
 * status [B]: 0 ok, 3 a snapshot taken, the final A or the final P holds a non-finite entry (zero A, P and hist).
 * M4Q_E_BADARG: B, E or N < 1, hist_every < 0, flags with unknown bits, a missing xs, u, A0, discount, models or status, neither P0
 * nor alpha > 0, a discount outside (0, 1] (or NaN), a count outside [0, N].
 * M4Q_E_UNSUPPORTED: no compiled shape, a plant-only shape, nz > 64 - (16, 1, 4), nz = 80.  Arguments are checked before the
 * device is asked for. */
#define M4Q_ONLINE_HERMITIAN 1
M4Q_API int m4q_online_dmdc_batch(int32_t B, int32_t dim_x, int32_t dim_u, int32_t order, int32_t E, int32_t N, const double* xs,
                       const double* u, int32_t u_per_instance, const double* u_scale, const int32_t* counts, const double* A0,
                       int32_t A0_per_instance, const double* P0, int32_t P0_per_instance, double alpha, const double* discount,
                       int32_t discount_per_instance, int32_t flags, int32_t hist_every, double* models, double* P, double* hist,
                       double* innov, int32_t* status);

/* replaces the whole mpc() loop body (mpc.py:161-292) for B closed loops, all n_steps in one launch.
 * models [B|1][n][n(1+P)] c, x0 [B][n] c, X_targ [B|1][cols][n] c, U_targ [B|1][cols][m] r,
 * Q, Qf [n][n] c, R [m][m] c, op0/ops as in m4q_plant_step_batch
 * -> xs [B][n_steps+1][n] c, us [B][n_steps][m] r, exit_codes [B], steps_done [B], qp_solves [B][n_steps] */
M4Q_API int m4q_mpc_batch(const m4q_problem* p, int32_t B, const double* models, const double* x0, const double* X_targ,
                  const double* U_targ, const double* Q, const double* R, const double* Qf, const double* op0,
                  const double* ops, double* xs, double* us, int32_t* exit_codes, int32_t* steps_done,
                  int32_t* qp_solves);

/* ---- resident session (inputs stay in HBM; used by bench.py and by step-wise host plants) ---- */
typedef struct m4q_session m4q_session;

enum m4q_field {
  M4Q_F_MODELS = 0,
  M4Q_F_X0 = 1,
  M4Q_F_X_TARG = 2,
  M4Q_F_U_TARG = 3,
  M4Q_F_Q = 4,
  M4Q_F_R = 5,
  M4Q_F_QF = 6,
  M4Q_F_OP0 = 7,
  M4Q_F_OPS = 8,
  M4Q_F_XS = 9,         /* [B][n_steps+1][n] c */
  M4Q_F_US = 10,        /* [B][n_steps][m] r */
  M4Q_F_CODES = 11,     /* [B] i32 */
  M4Q_F_STEPS_DONE = 12,/* [B] i32 */
  M4Q_F_QP_SOLVES = 13, /* [B][n_steps] i32 */
  M4Q_F_X_GUESS = 14,   /* [B][T+1][n] c   SQP guess carried between MPC steps (mpc.py:141,228,271) */
  M4Q_F_U_GUESS = 15,   /* [B][T][m] r     together with XS/US/CODES this is the whole resumable state */
  M4Q_F_COUNT = 16
};

/* device < 0: keep the current device */
M4Q_API int m4q_session_create(const m4q_problem* p, int32_t B, int32_t device, m4q_session** out);
M4Q_API void m4q_session_destroy(m4q_session* s);
/* size in bytes the session expects for a field */
M4Q_API size_t m4q_session_field_bytes(const m4q_session* s, int32_t field);
/* host -> device / device -> host copy of a whole field (synchronous w.r.t. the session stream) */
M4Q_API int m4q_session_upload(m4q_session* s, int32_t field, const void* host, size_t bytes);
M4Q_API int m4q_session_download(m4q_session* s, int32_t field, void* host, size_t bytes);
/* upload/download one MPC step's column of XS for every instance: host [B][n] c (host plants) */
M4Q_API int m4q_session_put_state(m4q_session* s, int32_t step, const void* host);
M4Q_API int m4q_session_get_state(m4q_session* s, int32_t step, void* host);
/* fill M4Q_F_MODELS on the device from continuous-time generators (as m4q_discretize_batch; dt, generators
 * [B|1][1+m][n][n] c and scales [B][1+m] r (or NULL) are host buffers): no model ever crosses PCIe */
M4Q_API int m4q_session_build_models(m4q_session* s, double dt, const double* generators, int32_t gen_per_instance,
                             const double* scales);
/* raw device pointer of a field (for collectives on the results); NULL if unknown */
M4Q_API void* m4q_session_device_ptr(m4q_session* s, int32_t field);
/* use caller-owned DEVICE memory for an output field (XS, US, CODES, STEPS_DONE, QP_SOLVES) */
M4Q_API int m4q_session_bind_output(m4q_session* s, int32_t field, void* device_ptr, size_t bytes);
/* enqueue MPC steps [step_begin, step_end) on the session stream; step_begin == 0 re-initialises the guesses */
M4Q_API int m4q_session_run(m4q_session* s, int32_t step_begin, int32_t step_end);
M4Q_API int m4q_session_sync(m4q_session* s);
/* mark instances finished from the host (exit_condition, mpc.py:289-292): codes [B] i32, nonzero = stop */
M4Q_API int m4q_session_set_codes(m4q_session* s, const int32_t* codes);
/* exit condition the closed-loop kernel evaluates itself (mpc.py:289-292 for one family of conditions), for every member on its own,
 * after each MPC step that completed with code 0:
 *     q = Re((x - f)^H W (x - f)),  fires when q < thr (M4Q_EXIT_BELOW) or q > thr (M4Q_EXIT_ABOVE)
 * with x = xs[step] (M4Q_EXIT_PREV: the state the step started from) or xs[step + 1] (M4Q_EXIT_NEXT: the state it produced - on a
 * step that is not measured, the model's prediction), exactly as stored in XS.  A member it fires for ends with exit code 1 and
 * steps_done = step: that step's entries are dropped, as mpc.py:298-304 drops them.  W [n][n] c (not required to be Hermitian),
 * target [B|1][n] c, thr [B|1] r are host buffers, copied into buffers the session owns; the condition holds for the launches that
 * follow.  mode 0 clears it.  M4Q_E_BADARG for any other combination of bits or a missing array, M4Q_E_UNSUPPORTED for a
 * M4Q_PLANT_NONE session (its host supplies the states and evaluates its own condition). */
#define M4Q_EXIT_PREV 1
#define M4Q_EXIT_NEXT 2
#define M4Q_EXIT_BELOW 4
#define M4Q_EXIT_ABOVE 8
M4Q_API int m4q_session_set_exit(m4q_session* s, int32_t mode, const double* W, const double* target, int32_t target_per_instance,
                                 const double* thr, int32_t thr_per_instance);
/* measurement noise the closed-loop kernel draws itself (QExperiment.set_sigma, experiment.py:188-212, for whole ensembles): on every
 * measured step,  xs[b][step + 1] += e(seed, member_base + b, step + 1)  before the state is stored, so every later linearisation,
 * QP, plant step and exit condition sees it.  The generator is counter-based (Philox4x32-10 -> two 53-bit uniforms -> Box-Muller;
 * mpc4quantum_amd/noise.py is its normative definition): a draw depends on the seed, the GLOBAL member index, the column of XS and
 * the component, and on nothing else - not the launch, the split of a run into launches, the resident row or the rank.
 *   M4Q_NOISE_IID        e = sigma z, z a unit complex normal per component (the reference's noise as written).  It does not keep
 *                        a density matrix Hermitian: such a session runs the complex path (m4q_session_path 0).
 *   M4Q_NOISE_HERMITIAN  e = sigma ((Z + Z^H) / 2 - (Re tr Z / d) I) with Z[a][b] = z of component a d + b: Hermitian and
 *                        traceless, every arithmetic path stays available.  Not for M4Q_PLANT_PROCESS (no density matrix).
 * sigma: host buffer of 1 or B (sigma_per_instance) entries, finite and >= 0, copied.  Call it before the session's first
 * m4q_session_run; a later call may change sigma, seed and member_base but not mode (the arithmetic path depends on it).
 * mode 0 clears the setting.  M4Q_E_BADARG for a null session, another mode, a missing, negative or non-finite sigma, a
 * M4Q_PLANT_NONE session (its host supplies the states), M4Q_NOISE_HERMITIAN on a process plant, or a forbidden change. */
#define M4Q_NOISE_IID 1
#define M4Q_NOISE_HERMITIAN 2
M4Q_API int m4q_session_set_noise(m4q_session* s, int32_t mode, const double* sigma, int32_t sigma_per_instance, uint64_t seed,
                                  uint64_t member_base);
/* the noise m4q_session_set_noise adds to xs[:, state_index] (state_index = step + 1 >= 1) of B members with n-dimensional states,
 * by the device function the closed loop calls: out [B][n] c (host).  n must be a dim_x with compiled kernels; M4Q_NOISE_HERMITIAN
 * needs n = d d. */
M4Q_API int m4q_noise_sample_batch(int32_t B, int32_t n, int32_t mode, const double* sigma, int32_t sigma_per_instance, uint64_t seed,
                                   uint64_t member_base, int32_t state_index, double* out);
/* Observed plants: the loop closes on x = observe(z) of a plant state z that the model does not describe (the reference's
 * QCoupledExperiment and QExperiment32; mpc4quantum_amd/observe.py is the normative definition).  z has n_p = d_p^2 entries and
 * evolves by M4Q_PLANT_HAMILTONIAN's arithmetic on d_p x d_p operators; x has n = dim_x entries.
 *   M4Q_OBSERVE_PARTIAL_TRACE  n_p = 16, n = 8: z = vec_r of a two-qubit state, x = [vec_r(tr_B rho), vec_r(tr_A rho)]
 *   M4Q_OBSERVE_QUBIT_BLOCK    n_p = 9,  n = 4: z = vec_r of a three-level state, x = vec_r(Bk / s), Bk its leading 2 x 2 block and
 *                              s = sqrt(|Bk|_F^2 + 2 |det Bk|) its trace norm (s = 0 gives NaN: the member ends with exit code 3)
 * An observed plant is a setting of an M4Q_PLANT_NONE session, not a plant_kind: m4q_session_create, m4q_plant_step_batch, the
 * rollouts and their gradients take the plant kinds above and nothing else; exit conditions and noise stay refused on such a session. */
#define M4Q_OBSERVE_PARTIAL_TRACE 1
#define M4Q_OBSERVE_QUBIT_BLOCK 2
/* x = observe(z) alone, by the kernel the loop calls: z [B][n_p] c, x [B][n] c (host).  M4Q_E_BADARG: B < 1, another kind, a
 * null pointer. */
M4Q_API int m4q_observe_batch(int32_t B, int32_t observe, const double* z, double* x);
/* op0 [B|1][d_p][d_p] c, ops [B|1][m][d_p][d_p] c (plant_per_instance), z0 [B][n_p] c: host buffers, copied.  Allocates the plant
 * states zs [B][n_steps + 1][n_p] (zero), writes zs[:, 0] = z0 and xs[:, 0] = observe(z0); the caller uploads the same observe(z0)
 * (m4q_observe_batch) as M4Q_F_X0.  M4Q_E_BADARG, before any device work: a session whose plant_kind is not M4Q_PLANT_NONE,
 * measure_freq > 1, a dim_x that is not the kind's n, a null pointer, a call after the session's first run. */
M4Q_API int m4q_session_set_observed_plant(m4q_session* s, int32_t observe, const double* op0, const double* ops,
                                           int32_t plant_per_instance, const double* z0);
/* for k in [step_begin, step_end): the launch of m4q_session_run(k, k + 1), then one kernel that - for every member that launch
 * completed step k for (exit code 0, steps_done = k + 1) - takes the plant step zs[k] -> zs[k + 1] under us[k] and stores
 * xs[k + 1] = observe(zs[k + 1]); every other member is left untouched.  All on the session's stream: no synchronisation, no copy.
 * Ranges are refused as m4q_session_run refuses them. */
M4Q_API int m4q_session_run_observed(m4q_session* s, int32_t step_begin, int32_t step_end);
/* download / upload (restore) zs [B][n_steps + 1][n_p] c; both synchronise and check the watchdog, as m4q_session_download does */
M4Q_API int m4q_session_plant_states(m4q_session* s, void* host, size_t bytes);
M4Q_API int m4q_session_put_plant_states(m4q_session* s, const void* host, size_t bytes);
/* kernel time of the launches since the last call, from HIP events on the session stream */
M4Q_API int m4q_session_kernel_ms(m4q_session* s, double* total_ms, int32_t* launches);
/* arithmetic path the uploaded problem will run on: 0 complex, 1 real (Hermitian operator basis, d*d coordinates),
 * 2 real on the d*d - 1 traceless coordinates, 3 the same with the sweeps on matrix-core tiles, 4 the traceless clipped solve on
 * shared generators (M4Q_OPT_NO_SG) */
M4Q_API int m4q_session_path(const m4q_session* s);
/* M4Q_QP_EXACT_BOX sessions: counters of the last launch - out[0] QP solves, out[1] Riccati sweeps with pinned
 * controls, out[2] ratio-test steps, out[3..5] solves ended by the KKT test / at working precision / by the iteration
 * cap (the last two leave a feasible, possibly sub-optimal point).  All zero for a clipped-Riccati session. */
M4Q_API int m4q_session_qp_stats(m4q_session* s, int64_t* out6);
/* resident bytes and launch geometry, for reports */
M4Q_API int m4q_session_info(const m4q_session* s, int64_t* hbm_bytes, int32_t* grid, int32_t* lds_bytes);
/* final-state-only results: copy xs[:, n_steps, :] of the session's state history into dst_dev [B][n] c (device memory),
 * enqueued on the session stream behind the launches queued so far */
M4Q_API int m4q_session_copy_final_state(m4q_session* s, void* dst_dev);
/* the watchdog flag (0 / 1, int32) of the launches queued so far into dst_dev (device memory), on the session stream: the
 * status word of a gather buffer, so that the gathering rank sees M4Q_E_TIMEOUT of any rank in the bytes it receives */
M4Q_API int m4q_session_copy_status(m4q_session* s, void* dst_dev);

/* ---- ensemble sharding over the GPUs of one node: one process per GPU, ONE gather of results at the end ----------
 * The reference has no counterpart: mpc4quantum/mpc.py:128-304 runs one closed loop and has no cross-instance data
 * flow, which is exactly why an ensemble shards with no collective on the data path.  The communicator is RCCL
 * (librccl.so, loaded on first use) over xGMI; the unique id travels between the processes by whatever the launcher
 * offers (mpc4quantum_amd/distributed.py: a file keyed by the launcher's MASTER_PORT). */
typedef struct m4q_comm m4q_comm;
#define M4Q_UNIQUE_ID_BYTES 128
#define M4Q_E_COMM (-1005) /* librccl.so missing, or an RCCL call failed (m4q_last_error() has ncclGetErrorString) */

/* rank 0: a fresh RCCL unique id (ncclGetUniqueId), id128 = M4Q_UNIQUE_ID_BYTES caller-owned bytes */
M4Q_API int m4q_comm_unique_id(void* id128);
/* every rank, same id: ncclCommInitRank on `device` (< 0: the current one); collective - returns when all ranks joined */
M4Q_API int m4q_comm_create(int32_t rank, int32_t world, const void* id128, int32_t device, m4q_comm** out);
M4Q_API void m4q_comm_destroy(m4q_comm* c);
/* the one collective of a job: ncclGather of `bytes` bytes from every rank's send_dev into recv_dev on rank dst
 * (world * bytes there; ignored elsewhere).  Enqueued on the communicator's own stream BEHIND everything queued so far
 * on `after`'s stream (after may be NULL), so the kernel that fills send_dev needs no host synchronisation; `slot`
 * (0..7) names the completion event m4q_comm_wait blocks on - two buffers can alternate so that the gather of run k
 * travels under the kernel of run k+1. */
M4Q_API int m4q_comm_gather(m4q_comm* c, m4q_session* after, const void* send_dev, void* recv_dev, size_t bytes, int32_t dst,
                            int32_t slot);
/* host blocks until the gather last enqueued under `slot` has completed (slot < 0: every collective enqueued so far) */
M4Q_API int m4q_comm_wait(m4q_comm* c, int32_t slot);
/* small host-side reductions for reports and fences (op 0 = sum, 1 = max) over n <= 64 doubles, in place;
 * n = 0 is a barrier.  Blocks until done. */
M4Q_API int m4q_comm_allreduce_f64(m4q_comm* c, double* inout_host, int32_t n, int32_t op);

/* device memory owned by the library (gather buffers): zero-filled; device < 0 = the current one */
M4Q_API int m4q_device_alloc(size_t bytes, int32_t device, void** out);
M4Q_API int m4q_device_free(void* dev);
M4Q_API int m4q_device_read(void* host, const void* dev, size_t bytes);  /* blocking device -> host copy */
M4Q_API int m4q_device_write(void* dev, const void* host, size_t bytes); /* blocking host -> device copy */

#ifdef __cplusplus
}
#endif
#endif /* M4Q_H */

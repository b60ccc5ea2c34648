// m4q_args.h - plain argument blocks passed by value to the kernels, shared by the per-shape
// kernel translation units (m4q_kernels.hip) and the host side of the C ABI (m4q_capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "m4q_paths.h"      // enum Path, enum Coords

// Pointer fields of the argument blocks: plain pointers for the host pass; for the device pass the SAME 8 bytes typed as
// global-address-space pointers, so that a pointer read out of the kernarg segment at its point of use (kargs() in
// m4q_kernels.hip) still yields global_load / global_store instructions, not flat ones.
// (Only in the kernel translation units, which define M4Q_KERNEL_TU: the host code of m4q_capi.hip, which fills these fields, is
// also parsed by its device pass.)
#if defined(__HIP_DEVICE_COMPILE__) && defined(M4Q_KERNEL_TU)
#define M4Q_GLOBAL __attribute__((address_space(1)))
#else
#define M4Q_GLOBAL
#endif
#define M4Q_P(T) T M4Q_GLOBAL*

namespace m4q {

struct cplx;

// QP semantics flags (mirrored in include/m4q.h: M4Q_QP_*; the last two are internal, set by the host)
enum : int {
  QP_REF_LQR = 1,   // reproduce lqr.py as written (no Delta, xbar_{t+1}==xbar_t, cost built on xbar, absolute cost)
  QP_DU_BAND = 2,   // clip the first control to u_prev +- du as well (optimize.py:29-30)
  QP_EXACT_BOX = 4, // solve the box-constrained QP to optimality (projected Newton) instead of clipping the Riccati rollout
  QP_TARG_CONST = 256,   // internal (set by the host when every column of X_targ is the same): xbar_t does not depend on t
  QP_NO_TILE = 512,      // internal (the session may not take PATH_TILE: the exact traceless kernel holds both forms of the pinned sweep)
};

constexpr Coords coords_of(Path p) { return p == PATH_COMPLEX ? COORDS_COMPLEX : p == PATH_REAL ? COORDS_HERM : COORDS_TRACELESS; }

// The plant operators of a launch: op0 [B|1][k][k] and ops [B|1][m][k][k] complex, k the side the plant kind gives them (n for the
// generator, d with d^2 = n for the Hamiltonian, d with d^4 = n for the process plant; d_p for an observed plant).  Per member or
// shared: the strides are k k and m k k, or both 0 when shared.  Every block that steps a plant holds one as its member `plant`,
// where the four fields stood before; the kernels read a.plant.op0 ... in place (a function around the reads changes their code).
struct PlantOps {
  M4Q_P(const cplx) op0; long op0_stride;
  M4Q_P(const cplx) ops; long ops_stride;
};

// Arrays marked S are complex (cplx) on the general path and double on the real path (models that preserve
// Hermiticity, expressed in the Hermitian operator basis of m4q_mpc.h); the host picks the kernel.
struct MpcArgs {
  int B, T, n_steps, max_iter, warm_start, flags, step_begin, step_end, measure_freq;
  double dt, sat, du, ls_tol;
  M4Q_P(const void) models;  long model_stride;   // S [B|1][n][n(1+P)]
  M4Q_P(const cplx) x0c;                          // [B][n] complex, as given (becomes xs[:, 0])
  M4Q_P(const void) x0s;                          // S [B][n]
  M4Q_P(const void) x_targ;  long xt_stride;      // S [B|1][cols][n]
  M4Q_P(const double) u_targ; long ut_stride;     // [B|1][cols][m]
  M4Q_P(const void) Q; M4Q_P(const void) Qf; M4Q_P(const void) R;            // S
  M4Q_P(const double) Cq; M4Q_P(const double) Cqf; M4Q_P(const double) Cr;   // line-search blocks (mpc.py:103-116)
  M4Q_P(const double) Wls;                        // [2n + 2n + 2m] diagonals of those blocks, or nullptr if one is not diagonal
  PlantOps plant;                                 // (a PLANT_NONE session: both point at Q, strides 0 - never read)
  M4Q_P(cplx) xs; M4Q_P(double) us; M4Q_P(int) codes; M4Q_P(int) steps_done; M4Q_P(int) qp_solves;
  M4Q_P(cplx) Xg; M4Q_P(double) Ug;                     // per-instance SQP guess  [B][T+1][n] complex, [B][T][m] (resumable state)
  // per resident row (grid*4 of them): working guess followed by the QP solution (S [2][rows][T+1][n], [2][rows][T][m]), gains (S)
  M4Q_P(void) ws_Xg; M4Q_P(double) ws_Ug; M4Q_P(void) ws_gains;
  M4Q_P(int) queue;                               // 64 B zeroed before every launch: [0] next work item to hand out; [1] set by the watchdog;
                                            // as u64 [1..3]: exact-QP counters (solves, Newton iterations, arc trials)
  M4Q_P(int) head_done;                           // [B] set when an instance's head item (steps < 2) has been published; zeroed likewise
  unsigned long long deadline_ticks;        // watchdog: the launch abandons itself (queue[1] = 1) once s_memrealtime (100 MHz) has
                                            // advanced this far since the wavefront started; every wavefront reaches this exit
  // shared-generator sessions (PATH_SG): dt L_k on the recursion's coordinates, [1 + m][ns][ns] doubles, and the members' scales
  // [B][1 + m]; the kernel forms A_i = I + s_i0 dt L_0 itself and never reads `models`
  M4Q_P(const double) gens; M4Q_P(const double) scales;
  // exit condition (m4q_session_set_exit; device plants only): exit_mode is 0 (none) or one of EXIT_PREV / EXIT_NEXT with one of
  // EXIT_BELOW / EXIT_ABOVE.  q = Re((x - f)^H W (x - f)) of the stored state x = xs[step] (PREV) or xs[step + 1] (NEXT);
  // W [n][n] complex, f [B|1][n] complex (exit_tstride n or 0), thresholds [B|1] (exit_thr_stride 1 or 0)
  int exit_mode;
  M4Q_P(const cplx) exit_W; M4Q_P(const cplx) exit_target; long exit_tstride;
  M4Q_P(const double) exit_thr; long exit_thr_stride;
  // measurement noise (m4q_session_set_noise; device plants only): noise_mode is 0 (none), NOISE_IID or NOISE_HERMITIAN (m4q_noise.h).
  // On every measured step xs[b][step + 1] += the draw of (noise_seed, noise_member_base + b, step + 1, component) scaled by the
  // member's sigma [B|1] (noise_sigma_stride 1 or 0)
  int noise_mode;
  M4Q_P(const double) noise_sigma; long noise_sigma_stride;
  unsigned long long noise_seed, noise_member_base;
};
enum : int { EXIT_PREV = 1, EXIT_NEXT = 2, EXIT_BELOW = 4, EXIT_ABOVE = 8 };     // (mirrored in include/m4q.h: M4Q_EXIT_*)

struct LinArgs {
  int B, T;
  M4Q_P(const cplx) models; long model_stride;
  M4Q_P(const cplx) X; M4Q_P(const double) U;           // [B][T][n], [B][T][m]
  M4Q_P(cplx) A_ls; M4Q_P(cplx) B_ls; M4Q_P(cplx) D_ls;
};

struct QpArgs {
  int B, T, flags;
  double sat, du;
  M4Q_P(const cplx) x_init;
  M4Q_P(const cplx) X_bm; long xbm_stride;
  M4Q_P(const double) U_bm; long ubm_stride;
  M4Q_P(const cplx) Q_ls; M4Q_P(const cplx) R_ls;       // [T+1][n][n], [T][m][m]
  M4Q_P(const cplx) A_ls; M4Q_P(const cplx) B_ls; M4Q_P(const cplx) D_ls;
  M4Q_P(const double) u_prev;
  M4Q_P(cplx) X_opt; M4Q_P(double) U_opt; M4Q_P(double) cost; M4Q_P(cplx) gains;   // gains: caller buffer or workspace [B][T][n+1][m]
  // QP_EXACT_BOX workspace: two trajectory pairs in one allocation each (X_alt [2][B][T+1][n], U_alt [2][B][T][m]),
  // working set [B][T][m], sweeps per instance [B] (diagnostic, may be null)
  M4Q_P(cplx) X_alt; M4Q_P(double) U_alt; M4Q_P(double) pin_stat; M4Q_P(int) sweep_counts;
};

// discretize_homogeneous for B generator sets (vectorize.py:8-49).  gens: S [B|1][1+m][n][n] (row-major), scaled per
// instance by scales [B][1+m] when given; models: S [B][n][n(1+P)].
struct DiscArgs {
  int B;
  double dt;
  M4Q_P(const void) gens; long gen_stride;
  M4Q_P(const double) scales;
  M4Q_P(void) models;
};

struct PlantArgs {
  int B, kind;
  double dt;
  M4Q_P(const cplx) x; M4Q_P(const double) u;
  PlantOps plant;
  M4Q_P(cplx) x_next;
};

// Open-loop rollouts (m4q_plant_rollout_batch, m4q_model_rollout_batch): N held-control steps of B members in one launch.
// The member sees u_scale[b][k] u[t][k] (u_scale may be null); the plant advances by dts[t], the model by one of its own steps.
// xs_mode / q_mode: 0 nothing, 1 the last column ([B][n], [B]), 2 every column ([B][N + 1][n], [B][N + 1]; column 0 = x0).
// q = Re((x - f)^H W (x - f)), W [n][n] shared, f [B|1][n] (target_stride n or 0)
struct RollArgs {
  int B, N, kind, xs_mode, q_mode;
  M4Q_P(const double) dts;                         // [N] (plant rollout)
  M4Q_P(const cplx) x0;                            // [B][n]
  M4Q_P(const double) u; long u_stride;            // [B|1][N][m] (u_stride N m or 0)
  M4Q_P(const double) u_scale;                     // [B][m] or null
  PlantOps plant;                                  // (plant rollout)
  M4Q_P(const cplx) models; long model_stride;     // [B|1][n][n(1+P)], as LinArgs (model rollout)
  M4Q_P(const cplx) W; M4Q_P(const cplx) target; long target_stride;
  M4Q_P(cplx) xs; M4Q_P(double) q;
};

// Rollout gradients (m4q_plant_rollout_grad_batch, m4q_model_rollout_grad_batch; m4q_grad.h, grad.py is the definition).
// The forward pass is the rollout `roll` describes, with xs_mode 2 and xs the workspace [B][N + 1][n] the backward pass reads the
// states from; q_mode 1: J = q_N, 2: J = sum_t q_t.  grad [B][N][m] = dJ_b/du[t][k]; grad_scale [B][m] = dJ_b/du_scale[b][k] or null.
// reduce: the launcher then runs grad_reduce_kernel twice - members in chunks of GRAD_CHUNK into partial [chunks][N m + 1], the
// chunk partials into grad_mean [N][m] and q_mean [1] - with weights [B] (never null when reduce is set).
constexpr int GRAD_CHUNK = 256;
struct GradArgs {
  RollArgs roll;
  M4Q_P(double) grad; M4Q_P(double) grad_scale;
  int reduce;
  M4Q_P(const double) weights;
  M4Q_P(double) partial; M4Q_P(double) grad_mean; M4Q_P(double) q_mean;
};
// One pass of the ordered reduction (m4q_grad.h: grad_reduce): `count` rows in chunks of `chunk`
struct GradReduceArgs {
  int count, chunk, nm, q_cols;
  M4Q_P(const double) vals; long row_stride;
  M4Q_P(const double) q;
  M4Q_P(const double) w;                           // [count] or null
  M4Q_P(double) out; long out_stride;              // element e < nm of chunk c -> out[c out_stride + e]
  M4Q_P(double) out_last; long last_stride;        // element nm of chunk c -> out_last[c last_stride]
};

// Plant-parameter gradient (m4q_plant_rollout_param_grad_batch; m4q_plant_param.h, plant_param.py is the definition).  The forward
// pass is the rollout `roll` describes, with xs the workspace [B][N + 1][n] (roll.W is the objective's W; roll.target, roll.q and
// the two modes are unused).  Objective: J_b = sum_t col_w[t] Re((x_t - y_t)^H W (x_t - y_t)), y = data, t ascending from 0.0; a
// column whose weight is 0 is skipped.  The kernel is compiled for PT directions: the p matrices of dirs and - PT > p, then
// PT = p + m - the m drive gains.  grad_theta [B][p] = dJ_b/dtheta_j, grad_scale [B][m] = dJ_b/du_scale[b][k] (PT > p).
struct ParamGradArgs {
  RollArgs roll;
  int p;
  M4Q_P(const cplx) dirs; long dirs_stride;        // [B|1][p][d][d] (dirs_stride p d d or 0)
  M4Q_P(const cplx) data; long data_stride;        // [B|1][N + 1][n] (data_stride (N + 1) n or 0)
  M4Q_P(const double) col_w;                       // [N + 1]
  M4Q_P(double) J;                                 // [B]
  M4Q_P(double) grad_theta; M4Q_P(double) grad_scale;
};

// S control sequences shared by the ensemble, each rolled against all B members in one launch (m4q_plant_rollout_multi_batch and
// the line search of m4q_plant_robust_batch; m4q_rollout_multi.h).  Member b under sequence s sees u_scale[b][k] us[s][t][k]; its
// objective J[b][s] is q_N (q_mode 1) or sum_t q_t, t ascending from 0.0 (q_mode 2), q as RollArgs.  No state is stored.
// F non-null: the launcher then runs grad_reduce_kernel twice - members in chunks of GRAD_CHUNK into partial [chunks][S], the
// chunk partials into F [S] = sum_b weights[b] J[b][s] - with weights [B] (never null when F is set).
constexpr int MULTI_MAX_S = 8;
struct MultiArgs {
  int B, N, kind, S, q_mode;
  M4Q_P(const double) dts;                         // [N]
  M4Q_P(const cplx) x0;                            // [B][n]
  M4Q_P(const double) us;                          // [S][N][m]
  M4Q_P(const double) u_scale;                     // [B][m] or null
  PlantOps plant;
  M4Q_P(const cplx) W; M4Q_P(const cplx) target; long target_stride;
  M4Q_P(double) J;                                 // [B][S]
  M4Q_P(const double) weights;
  M4Q_P(double) partial; M4Q_P(double) F;
};
// ... through the members' models instead of their plants (m4q_model_rollout_multi_batch and the line search of
// m4q_model_robust_batch; m4q_model_multi.h): MultiArgs with the models, as RollArgs', where dts and the plant stood - a model
// advances by its own step.  A block of its own: MultiArgs is plant_rollout_multi_kernel's kernarg segment and stays as it is.
struct ModelMultiArgs {
  int B, N, S, q_mode;
  M4Q_P(const cplx) x0;                            // [B][n]
  M4Q_P(const double) us;                          // [S][N][m]
  M4Q_P(const double) u_scale;                     // [B][m] or null
  M4Q_P(const cplx) models; long model_stride;     // [B|1][n][n(1+P)] (model_stride n n (1 + P) or 0)
  M4Q_P(const cplx) W; M4Q_P(const cplx) target; long target_stride;
  M4Q_P(double) J;                                 // [B][S]
  M4Q_P(const double) weights;
  M4Q_P(double) partial; M4Q_P(double) F;
};

// The plant's own linearisation along trajectories (m4q_plant_linearize_batch; m4q_plant_lin.h, plant_linearize.py is the
// definition): the work unit is a (member, point) pair, B T of them.  Member b at point t: state X[b][t], controls U[b|.][t] as the
// caller passed them (the member sees u_scale[b][k] u_k; u_scale may be null), step length dts[t].  Each output may be null.
// PlantTraj is that input side - the plant and the trajectories it is linearised along - which PlantQpArgs holds too.
struct PlantTraj {
  M4Q_P(const double) dts;                         // [T]
  M4Q_P(const cplx) X;                             // [B][T][n]
  M4Q_P(const double) U; long u_stride;            // [B|1][T][m] (u_stride T m or 0)
  M4Q_P(const double) u_scale;                     // [B][m] or null
  PlantOps plant;
};
struct PlantLinArgs {
  int B, T, kind;
  PlantTraj traj;
  M4Q_P(cplx) A_ls; M4Q_P(cplx) B_ls; M4Q_P(cplx) D_ls;      // [B][T][n][n], [B][T][n][m], [B][T][n], as LinArgs
};

// The QP of QpArgs on the linearisation PlantLinArgs describes, in two launches on one stream and no host in between
// (m4q_plant_quad_program_batch; m4q_plant_qp.h): plant_factor_kernel writes U_t, B_t and Delta_t of every (member, point) pair
// into the three workspaces, plant_qp_kernel sweeps each member over them.  x_init null: member b starts from traj.X[b][0].
struct PlantQpArgs {
  int B, T, kind, flags;
  double sat, du;
  PlantTraj traj;                                  // the plant side: PlantLinArgs'
  M4Q_P(const cplx) x_init;                        // the QP side, as QpArgs ([B][n] or null)
  M4Q_P(const cplx) X_bm; long xbm_stride;
  M4Q_P(const double) U_bm; long ubm_stride;
  M4Q_P(const cplx) Q_ls; M4Q_P(const cplx) R_ls;
  M4Q_P(const double) u_prev;
  M4Q_P(cplx) U_ws; M4Q_P(cplx) B_ws; M4Q_P(cplx) D_ws;      // workspaces [B][T][d][d], [B][T][n][m], [B][T][n]: never copied back
  M4Q_P(cplx) X_opt; M4Q_P(double) U_opt; M4Q_P(double) cost; M4Q_P(cplx) gains;
  M4Q_P(cplx) X_alt; M4Q_P(double) U_alt; M4Q_P(double) pin_stat; M4Q_P(int) sweep_counts;   // QP_EXACT_BOX, as QpArgs
};

// The step of the SQP and of the iLQR on the plant itself (m4q_plant_sqp_batch, m4q_plant_ilqr_batch; m4q_plant_step.h, plant_sqp.py
// is the definition), launched between two QPs of PlantQpArgs on the same device buffers: U is that block's U (u_stride T m), X_lin
// its X, x0 its x_init, U_qp its U_opt, gains its gains.  iter < 0: the initial roll of clip(U0); iter >= 0: the line search of
// iteration iter over `steps` candidates, the member's decision and the hand-over of the accepted trajectory.  closed 0: the
// candidates are points of the line from U to U_qp (the SQP); 1: the QP's law run on the plant around the iterate (X_lin, U) (the
// iLQR).  Like kind it picks the kernel: the launcher reads it, no kernel does.  status: 0 running (at the end: iterations used
// up), 1 converged, 2 no descent, 3 the first cost was not finite; a member whose status is not 0 keeps what it has.
struct PlantStepArgs {
  int B, T, kind, flags, iter, iters, steps, closed;
  double sat, du, tol;
  M4Q_P(const double) dts;                         // the plant side, as PlantTraj but for the guess: the iterate is below
  M4Q_P(const cplx) x0;                            // [B][n]
  M4Q_P(const double) U0; long u0_stride;          // [B|1][T][m] (u0_stride T m or 0): read by the initial roll alone
  M4Q_P(const double) u_scale;
  PlantOps plant;
  M4Q_P(const cplx) X_bm; long xbm_stride;         // the cost and the bounds, as PlantQpArgs
  M4Q_P(const double) U_bm; long ubm_stride;
  M4Q_P(const cplx) Q_ls; M4Q_P(const cplx) R_ls;
  M4Q_P(const double) u_prev;
  M4Q_P(const double) U_qp;                        // [B][T][m]: the QP's U_opt (closed: what a pinned control of the exact mode goes to)
  M4Q_P(const cplx) gains;                         // [B][T][n + 1][m]: the QP's rows, read when closed
  M4Q_P(double) U; M4Q_P(cplx) X_lin; M4Q_P(cplx) X;                   // the iterate: [B][T][m], [B][T][n], [B][T + 1][n]
  M4Q_P(double) cost; M4Q_P(double) cost_hist; M4Q_P(double) alpha_hist;   // [B], [B][iters + 1], [B][iters]
  M4Q_P(int) n_iter; M4Q_P(int) status;            // [B]
};

// A stored feedback law closing the loop of a rollout (m4q_plant_feedback_batch, m4q_model_feedback_batch; m4q_feedback.h,
// feedback.py is the definition).  `roll` is the rollout without its control sequence (roll.u is u_ref, roll.u_stride its
// stride): at step t the member commands u_t = clip(Re(K_t [x_t - x_ref[t] ; 1]) + u_ref[t]) and sees u_scale[b][k] u_t[k].
// The law is per member or shared as a whole: law_per 1 or 0 multiplies the strides N (n + 1) m, N n and N m.
// du_band: the band p +- du around the control applied before (u_prev [B|1][m] at t = 0; u_prev_stride m or 0) joins the box.
// noise_mode etc.: as MpcArgs', the draw of (seed, member_base + b, t + 1, component) is added to x_{t+1}.
struct FeedbackArgs {
  RollArgs roll;
  M4Q_P(const cplx) gains; M4Q_P(const cplx) x_ref; M4Q_P(const double) u_ref; int law_per;
  double sat, du; int du_band;
  M4Q_P(const double) u_prev; long u_prev_stride;
  int noise_mode;
  unsigned long long seed, member_base;
  M4Q_P(const double) sigma; long sigma_stride;    // [B|1]
  M4Q_P(double) us;                                // [B][N][m] or null
  M4Q_P(int) clipped;                              // [B] or null
  M4Q_P(int) status;                               // [B]: 0 ok, 3 a state or control was not finite
};

// m4q_dmdc_fit_batch: the truncated least-squares DMDc fit of B members from E experiments of N steps each (m4q_fit.h; fit.py is
// the definition).  The member sees u_scale[b][k] u[e][t][k], as in the rollouts.  rconds live in device memory: the kernel indexes
// them at run time.
struct FitArgs {
  int B, E, N, R;
  M4Q_P(const cplx) xs;                            // [B][E][N + 1][n]
  M4Q_P(const double) u; long u_stride;            // [B|1][E][N][m] (u_stride E N m or 0)
  M4Q_P(const double) u_scale;                     // [B][m] or null
  M4Q_P(const double) rconds;                      // [R]
  M4Q_P(cplx) models;                              // [R][B][n][n(1+P)]
  M4Q_P(int) ranks;                                // [R][B] or null
  M4Q_P(double) svals;                             // [B][n(1+P)] or null
  M4Q_P(int) status;                               // [B]: 0 ok, 1 the Jacobi iteration hit its cap, 3 non-finite data
};

// m4q_dmdc_refit_batch, m4q_dmdc_refit_qr_batch: the same fit against a prior model, A0 + the truncated fit of Y - A0 Z (fit.py's
// last part).  Member b takes the first counts[b] steps of each experiment (N when counts is null), weighted discount^(age).
struct RefitArgs {
  FitArgs fit;
  M4Q_P(const int) counts;                         // [B] or null
  M4Q_P(const cplx) A0; long A0_stride;            // [B|1][n][nz]
  M4Q_P(const double) discount; long discount_stride;     // [B|1]
};

// m4q_online_dmdc_batch: OnlineDMDc.fit_iteration for every snapshot of B members (m4q_online.h; online.py is the definition).
// The snapshots are FitArgs'; member b takes the first counts[b] steps of each experiment (N when counts is null).
struct OnlineArgs {
  int B, E, N, hist_every;
  double alpha;                                    // P0 = alpha I when P0 is null
  M4Q_P(const cplx) xs;                            // [B][E][N + 1][n]
  M4Q_P(const double) u; long u_stride;            // [B|1][E][N][m] (u_stride E N m or 0)
  M4Q_P(const double) u_scale;                     // [B][m] or null
  M4Q_P(const int) counts;                         // [B] or null
  M4Q_P(const cplx) A0; long A0_stride;            // [B|1][n][nz]
  M4Q_P(const cplx) P0; long P0_stride;            // [B|1][nz][nz] or null
  M4Q_P(const double) discount; long discount_stride;     // [B|1]
  M4Q_P(cplx) models;                              // [B][n][nz]
  M4Q_P(cplx) P;                                   // [B][nz][nz] or null
  M4Q_P(cplx) hist;                                // [E N / hist_every][B][n][nz]; null when hist_every is 0
  M4Q_P(double) innov;                             // [B][E N] or null
  M4Q_P(int) status;                               // [B]: 0 ok, 3 non-finite data or state
};

// noise.py's sample() for B members at one state_index (m4q_noise_sample_batch): out [B][n] complex
struct NoiseArgs {
  int B, mode;
  unsigned state_index;
  unsigned long long seed, member_base;
  M4Q_P(const double) sigma; long sigma_stride;   // [B|1]
  M4Q_P(cplx) out;
};

// Observed plants (m4q_observe.h; observe.py is the definition): the plant state z has n_p = d_p^2 entries and evolves by the
// Hamiltonian plant's arithmetic, the loop sees x = observe(z) of n = dim_x entries.  (mirrored in include/m4q.h: M4Q_OBSERVE_*)
enum : int { OBSERVE_PARTIAL_TRACE = 1, OBSERVE_QUBIT_BLOCK = 2 };
constexpr int observe_np(int kind) { return kind == OBSERVE_PARTIAL_TRACE ? 16 : kind == OBSERVE_QUBIT_BLOCK ? 9 : 0; }
constexpr int observe_dp(int kind) { return kind == OBSERVE_PARTIAL_TRACE ? 4 : kind == OBSERVE_QUBIT_BLOCK ? 3 : 0; }
constexpr int observe_n(int kind) { return kind == OBSERVE_PARTIAL_TRACE ? 8 : kind == OBSERVE_QUBIT_BLOCK ? 4 : 0; }

// x = observe(z) for B members (m4q_observe_batch; xs[:, 0] of a session): member b reads z + b z_stride, writes x + b x_stride
struct ObserveArgs {
  int B, kind;
  M4Q_P(const cplx) z; long z_stride;              // n_p entries each
  M4Q_P(cplx) x; long x_stride;                    // n entries each
};

// One MPC step of an observed plant, between two closed-loop launches of a PLANT_NONE session (m4q_session_run_observed): for
// every member with codes[b] == 0 and steps_done[b] == step + 1 - the launch just before completed that step - one plant step
// from zs[b][step] under us[b][step] into zs[b][step + 1], and its observation into xs[b][step + 1].  Other members: untouched.
struct ObsPlantArgs {
  int B, kind, step, n_steps;
  double dt;
  M4Q_P(const int) codes; M4Q_P(const int) steps_done;
  M4Q_P(const double) us;                          // [B][n_steps][m]
  PlantOps plant;                                  // (k = d_p)
  M4Q_P(cplx) zs;                                  // [B][n_steps + 1][n_p]
  M4Q_P(cplx) xs;                                  // [B][n_steps + 1][n]
};

// one entry per compiled (dim_x, dim_u, order)
struct ShapeOps {
  int nx, nu, order, np, d;
  int has_tile;                                                     // the tile form of the backward sweep is built for this shape (PATH_TILE)
  int has_sg;                                                       // the shared-generator form of the clipped traceless kernel (PATH_SG)
  int plant_only;                                                   // only plant_kernel is built (m4q_shapes.inc): serves m4q_plant_step_batch
  int (*mpc_lds_bytes)(int plant_kind, Path path, int exact_qp);   // dynamic LDS of the fused kernel's launch
  int (*launch_mpc)(const MpcArgs&, int plant_kind, Path path, int grid, hipStream_t);
  int (*launch_linearize)(const LinArgs&, hipStream_t);
  int (*launch_qp)(const QpArgs&, hipStream_t);
  int (*launch_plant)(const PlantArgs&, hipStream_t);
  int (*launch_discretize)(const DiscArgs&, Coords coords, hipStream_t);
  int (*power_list)(int32_t* out);
  int (*occupancy)(int plant_kind, Path path, int exact_qp);       // resident workgroups per CU of the fused kernel
  int (*launch_noise)(const NoiseArgs&, hipStream_t);             // (depends on dim_x alone)
  int (*launch_plant_rollout)(const RollArgs&, hipStream_t);      // (square shapes, plant-only ones included)
  int (*launch_model_rollout)(const RollArgs&, hipStream_t);      // (every shape with a model)
  int fit_lds_bytes;                                              // dynamic LDS of dmdc_fit_kernel; 0: the shape has none (no model, or
  int (*launch_fit)(const FitArgs&, hipStream_t);                 // its layout does not fit one workgroup's LDS)
  int online_lds_bytes;                                           // ... of online_dmdc_kernel, likewise
  int (*launch_online)(const OnlineArgs&, int hermitian, hipStream_t);
  int (*launch_plant_grad)(const GradArgs&, hipStream_t);          // (square shapes, plant-only ones included; no generator plant)
  int (*launch_model_grad)(const GradArgs&, hipStream_t);          // (every shape with a model)
  int observe_kind;                                                // the observation whose loop state has this dim_x (0: none)
  int (*launch_observe)(const ObserveArgs&, hipStream_t);          // (shapes with an observe_kind; depends on dim_x alone)
  int (*launch_observed_plant)(const ObsPlantArgs&, hipStream_t);  // (... and on dim_u: the plant has the shape's controls)
  int (*launch_fit_qr)(const FitArgs&, hipStream_t);               // dmdc_fit_qr_kernel: the shapes and the LDS of launch_fit
  int (*launch_plant_feedback)(const FeedbackArgs&, hipStream_t);  // (the shapes of launch_plant_rollout)
  int (*launch_model_feedback)(const FeedbackArgs&, hipStream_t);  // (the shapes of launch_model_rollout)
  int (*launch_refit)(const RefitArgs&, hipStream_t);              // dmdc_refit_kernel, dmdc_refit_qr_kernel: the shapes and the
  int (*launch_refit_qr)(const RefitArgs&, hipStream_t);           // LDS of launch_fit
  int (*launch_plant_linearize)(const PlantLinArgs&, hipStream_t); // (the shapes of launch_plant_grad; no generator plant)
  int (*launch_plant_qp)(const PlantQpArgs&, hipStream_t);         // (square shapes that hold qp_kernel; no generator plant)
  int (*launch_plant_step)(const PlantStepArgs&, hipStream_t);     // (the shapes and plants of launch_plant_qp)
  int (*launch_plant_multi)(const MultiArgs&, hipStream_t);        // (the shapes and plants of launch_plant_grad)
  int (*launch_model_multi)(const ModelMultiArgs&, hipStream_t);   // (the shapes of launch_model_rollout)
  // plant_param_grad_kernel<PLANT, p_tot>: square shapes with the auxiliary kernels; no generator plant; (1 + p_tot) d <= 16
  int (*launch_plant_param_grad)(const ParamGradArgs&, int p_tot, hipStream_t);
};

// The blocks are the kernels' kernarg segments: a field that moves changes every kernel that reads the block.  Where the operator
// block stands, what follows it and the size of each block that holds one, as they were when the four fields stood there bare.
static_assert(std::is_standard_layout<PlantOps>::value && sizeof(PlantOps) == 32, "PlantOps: two pointers, two strides");
static_assert(offsetof(PlantOps, op0_stride) == 8 && offsetof(PlantOps, ops) == 16 && offsetof(PlantOps, ops_stride) == 24, "PlantOps");
static_assert(std::is_standard_layout<PlantTraj>::value && sizeof(PlantTraj) == 72 && offsetof(PlantTraj, plant) == 40, "PlantTraj");
#define M4Q_PIN_PLANT(T, plant, plant_at, next, next_at, size)                                                         \
  static_assert(std::is_standard_layout<T>::value && offsetof(T, plant) == plant_at && offsetof(T, next) == next_at && \
                    sizeof(T) == size, #T ": the layout of the kernarg segment moved")
M4Q_PIN_PLANT(MpcArgs, plant, 192, xs, 224, 432);
M4Q_PIN_PLANT(PlantArgs, plant, 32, x_next, 64, 72);
M4Q_PIN_PLANT(RollArgs, plant, 64, models, 96, 152);
M4Q_PIN_PLANT(MultiArgs, plant, 56, W, 88, 144);
M4Q_PIN_PLANT(PlantLinArgs, traj.plant, 56, A_ls, 88, 112);
M4Q_PIN_PLANT(PlantQpArgs, traj.plant, 72, x_init, 104, 256);
M4Q_PIN_PLANT(PlantStepArgs, plant, 96, X_bm, 128, 264);
M4Q_PIN_PLANT(ObsPlantArgs, plant, 48, zs, 80, 96);
#undef M4Q_PIN_PLANT
static_assert(sizeof(GradArgs) == 208 && sizeof(FeedbackArgs) == 288, "the blocks that hold a RollArgs");
// ... and the model twin of MultiArgs: what the reduction behind both reads (B, S, J, weights, partial, F) has the same names
static_assert(std::is_standard_layout<ModelMultiArgs>::value && sizeof(ModelMultiArgs) == 112, "ModelMultiArgs: four ints, twelve 8-byte fields");
static_assert(offsetof(ModelMultiArgs, x0) == 16 && offsetof(ModelMultiArgs, models) == 40 && offsetof(ModelMultiArgs, model_stride) == 48 &&
                  offsetof(ModelMultiArgs, W) == 56 && offsetof(ModelMultiArgs, J) == 80 && offsetof(ModelMultiArgs, F) == 104,
              "ModelMultiArgs: the layout of the kernarg segment moved");

}  // namespace m4q

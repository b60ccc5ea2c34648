"""plant_sqp_batch with a closed-loop line search: an iLQR on the plant itself, for whole ensembles in ONE device call
(m4q_plant_ilqr_batch).  The step is the QP of plant_quad_program_batch on the plant's own Jacobians along the current trajectory,
as in plant_sqp.py; the candidates of the line search are not points of the line from U to the QP's U_opt but the QP's gains run
on the true plant, with the gains staying on the device between the QP and the forward pass.

The definition is here, in NumPy and SciPy.  The loop, the statuses, the histories, the tol rule and the tie rule are those of
plant_sqp.py's docstring; only the candidates differ.  Per member, with (Xbar, Ubar) the iterate, rows [T, m, n + 1] and U_qp what
the QP at (Xbar[:T], Ubar) with x_init = x0 returns, xb, ub the targets and lo, hi the box with the du band on t = 0:

    candidate j, a = 2^-j:   x_0 = x0
      for t in 0 .. T-1, control k:
        pinned(t, k) = exact and (U_qp[t, k] >= hi[t, k] or U_qp[t, k] <= lo[t, k])
        free:    ff = Re(rows[t][k, :n] @ (Xbar_t - xb_t)) + Re(rows[t][k, n]) + ub[t, k] - Ubar[t, k]
                 fb = Re(rows[t][k, :n] @ (x_t - Xbar_t))
        pinned:  ff = U_qp[t, k] - Ubar[t, k];  fb = 0       (the slot of a pinned control holds its multiplier row, not a policy)
        u[t, k] = clip((Ubar[t, k] + a ff) + fb, lo, hi)
        x_{t+1} = plant step under u_scale * u[t]
      J_j = J(x, u)

a is a power of two, so Ubar + a ff is one rounding (an fma on the device), then one add.  x_0 is Xbar_0 bit for bit, so fb = 0 at
t = 0; at a = 1 a free control is clip(pi_t(x_t)), the QP's stored law on the true plant (feedback.py); as a -> 0 the candidate
is the iterate.  The accepted (U, X, J) are the candidate's.  gains=True: one more linearisation and QP at the returned point,
whatever the status."""
import numpy as np

from . import _lib
from .plant_sqp import _clip, _descent_batch, _descent_reference


def _closed_loop(mem, a, Xbar, Ubar, U_qp, rows):
    """The iLQR's candidate (the module's docstring): the QP's law run on the plant around the iterate, feed-forward scaled by a."""
    n, lo, hi = mem.n, mem.lo, mem.hi
    X, U = np.empty((mem.T + 1, n), dtype=np.complex128), np.empty((mem.T, mem.m))
    X[0] = mem.x0
    with np.errstate(all="ignore"):
        for t in range(mem.T):
            K = rows[t][:, :n]
            pinned = (U_qp[t] >= hi[t]) | (U_qp[t] <= lo[t]) if mem.exact else np.zeros(mem.m, dtype=bool)
            ff = np.where(pinned, U_qp[t], (K @ (Xbar[t] - mem.Xb[t])).real + rows[t][:, n].real + mem.Ub[t]) - Ubar[t]
            fb = np.where(pinned, 0.0, (K @ (X[t] - Xbar[t])).real)
            U[t] = _clip((Ubar[t] + a * ff) + fb, lo[t], hi[t])
            X[t + 1] = mem.step(X[t], U[t], t)
    return X, U, mem.cost(X, U)


def plant_ilqr_reference(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                         kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False, trace=None):
    """The definition of plant_ilqr_batch (same arguments), on the host: the module's loop, member by member, on
    plant_quad_program_reference's pieces and feedback._plant_step.  trace: as plant_sqp_reference's - one dict per (member,
    iteration) with "b", "i", "J" and "U" (the cost and the controls before), "U_qp", "Js" and "Us" (the candidates' costs and
    controls)."""
    return _descent_reference(_closed_loop, x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind,
                              u_scale, exact, gains, trace)


def plant_ilqr_batch(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                     kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False):
    """An iLQR on the plant's own dynamics for B members in ONE device call (m4q_plant_ilqr_batch): plant_sqp_batch with the
    candidates of its line search run in closed loop - the gains of each iteration's QP applied on the true plant around the
    current trajectory, the feed-forward part scaled by the step lengths 1, 1/2, ... (the module's docstring).  Neither method
    ends lower on every problem: both take the same arguments, so an ensemble can be run through both and compared.

    Arguments and the returned dict: exactly plant_sqp_batch's."""
    return _descent_batch("m4q_plant_ilqr_batch", x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev,
                          kind, u_scale, exact, gains)

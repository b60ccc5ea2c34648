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
from .feedback import _plant_step
from .plant_linearize import _clipped_member, _exact_member, _objective, _reference_points
from .plant_sqp import STATUS_CONVERGED, STATUS_ITERS, STATUS_NO_DESCENT, STATUS_NOT_FINITE, _clip, _sqp_common
from .rollout import _ptr


def plant_ilqr_reference(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                         kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False, trace=None):
    """The definition of plant_ilqr_batch (same arguments), on the host: the module's loop, member by member, on
    plant_quad_program_reference's pieces and feedback._plant_step.  trace: as plant_sqp_reference's - one dict per (member,
    iteration) with "b", "i", "J" and "U" (the cost and the controls before), "U_qp", "Js" and "Us" (the candidates' costs and
    controls)."""
    (x0, U0, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev, iters, steps,
     tol) = _sqp_common(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind, u_scale)
    B, n = x0.shape
    T, m = U0.shape[-2:]
    k = op0.shape[-1]
    o0, ok, u0 = op0.reshape(-1, k, k), ops.reshape(-1, m, k, k), U0.reshape(-1, T, m)
    out = {"X": np.empty((B, T + 1, n), dtype=np.complex128), "U": np.empty((B, T, m)), "cost": np.empty(B),
           "cost_hist": np.empty((B, iters + 1)), "alpha_hist": np.zeros((B, iters)), "n_iter": np.zeros(B, dtype=np.int32),
           "status": np.zeros(B, dtype=np.int32), "gains": np.empty((B, T, n + 1, m), dtype=np.complex128) if gains else None}
    solve = _exact_member if exact else _clipped_member
    for b in range(B):
        H0, Hs = o0[b if per else 0], ok[b if per else 0]
        sc = np.ones(m) if u_scale is None else u_scale[b]
        Xb, Ub = X_bm[b if bm_per else 0], U_bm[b if bm_per else 0]
        lo, hi = np.full((T, m), -float(sat)), np.full((T, m), float(sat))
        if band:
            lo[0], hi[0] = np.maximum(lo[0], u_prev[b] - du), np.minimum(hi[0], u_prev[b] + du)

        def cost(X, U):
            with np.errstate(all="ignore"):
                return _objective(X, U, Xb, Ub, Q_ls, R_ls)

        def roll(U):
            X = np.empty((T + 1, n), dtype=np.complex128)
            X[0] = x0[b]
            for t in range(T):
                X[t + 1] = _plant_step(kind, X[t], sc * U[t], H0, Hs, dts[t])
            return X, cost(X, U)

        def qp(X, U):
            A, Bm, D = _reference_points(X[None, :T], U[None], 1, sc[None], H0[None], Hs[None], 1, dts, kind)
            return solve(x0[b], Xb, Ub, Q_ls, R_ls, A[0], Bm[0], D[0], lo, hi)

        def closed_loop(a, Xbar, Ubar, U_qp, rows):
            X, U = np.empty((T + 1, n), dtype=np.complex128), np.empty((T, m))
            X[0] = x0[b]
            with np.errstate(all="ignore"):
                for t in range(T):
                    K = rows[t][:, :n]
                    pinned = (U_qp[t] >= hi[t]) | (U_qp[t] <= lo[t]) if exact else np.zeros(m, dtype=bool)
                    ff = np.where(pinned, U_qp[t], (K @ (Xbar[t] - Xb[t])).real + rows[t][:, n].real + Ub[t]) - Ubar[t]
                    fb = np.where(pinned, 0.0, (K @ (X[t] - Xbar[t])).real)
                    U[t] = _clip((Ubar[t] + a * ff) + fb, lo[t], hi[t])
                    X[t + 1] = _plant_step(kind, X[t], sc * U[t], H0, Hs, dts[t])
            return X, U, cost(X, U)

        U = _clip(u0[b if u_per else 0], lo, hi)
        X, J = roll(U)
        hist = [J]
        status = STATUS_ITERS if np.isfinite(J) else STATUS_NOT_FINITE
        if status == STATUS_ITERS:
            for i in range(iters):
                _, U_qp, _, rows = qp(X, U)
                best = None
                rec = dict(b=b, i=i, J=J, U=U, U_qp=U_qp, Js=[], Us=[])
                if trace is not None:
                    trace.append(rec)
                for j in range(steps):
                    a = 0.5 ** j
                    Xj, Uj, Jj = closed_loop(a, X, U, U_qp, rows)
                    rec["Js"].append(Jj)
                    rec["Us"].append(Uj)
                    if np.isfinite(Jj) and (best is None or Jj < best[0]):
                        best = (Jj, a, Uj, Xj)
                if best is None or not best[0] < J:
                    status = STATUS_NO_DESCENT
                    break
                dec, J_old = J - best[0], J
                J, a, U, X = best
                out["alpha_hist"][b, i] = a
                hist.append(J)
                out["n_iter"][b] += 1
                if dec <= tol * J_old:
                    status = STATUS_CONVERGED
                    break
        out["X"][b], out["U"][b], out["cost"][b], out["status"][b] = X, U, J, status
        out["cost_hist"][b] = hist + [J] * (iters + 1 - len(hist))
        if gains:
            out["gains"][b] = qp(X, U)[3].transpose(0, 2, 1)
    return out


def plant_ilqr_batch(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                     kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False):
    """An iLQR on the plant's own dynamics for B members in ONE device call (m4q_plant_ilqr_batch): plant_sqp_batch with the
    candidates of its line search run in closed loop - the gains of each iteration's QP applied on the true plant around the
    current trajectory, the feed-forward part scaled by the step lengths 1, 1/2, ... (the module's docstring).  Neither method
    ends lower on every problem: both take the same arguments, so an ensemble can be run through both and compared.

    Arguments and the returned dict: exactly plant_sqp_batch's."""
    (x0, U0, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev, iters, steps,
     tol) = _sqp_common(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind, u_scale)
    B, n = x0.shape
    T, m = U0.shape[-2:]
    flags = (_lib.QP_DU_BAND if band else 0) | (_lib.QP_EXACT_BOX if exact else 0)
    out = {"X": np.empty((B, T + 1, n), dtype=np.complex128), "U": np.empty((B, T, m), dtype=np.float64),
           "cost": np.empty(B, dtype=np.float64), "cost_hist": np.empty((B, iters + 1), dtype=np.float64),
           "alpha_hist": np.empty((B, iters), dtype=np.float64), "n_iter": np.empty(B, dtype=np.int32),
           "status": np.empty(B, dtype=np.int32), "gains": np.empty((B, T, n + 1, m), dtype=np.complex128) if gains else None}
    ip = lambda a: a.ctypes.data_as(_lib._ip)
    L = _lib.lib()
    _lib.check(L.m4q_plant_ilqr_batch(B, n, m, kind, T, _ptr(dts), _ptr(x0), _ptr(U0), u_per, _ptr(u_scale), _ptr(op0), _ptr(ops), per,
                                      int(flags), float(sat), float(du if band else 0.0), _ptr(X_bm), _ptr(U_bm), bm_per, _ptr(Q_ls),
                                      _ptr(R_ls), _ptr(u_prev), iters, steps, tol, _ptr(out["X"]), _ptr(out["U"]), _ptr(out["cost"]),
                                      _ptr(out["cost_hist"]), _ptr(out["alpha_hist"]), ip(out["n_iter"]), ip(out["status"]),
                                      _ptr(out["gains"])))
    return out

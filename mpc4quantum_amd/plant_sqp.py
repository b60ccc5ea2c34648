"""Controls optimised on the plant itself, for whole ensembles in ONE device call (m4q_plant_sqp_batch): a Gauss-Newton SQP whose
step is the QP of plant_quad_program_batch on the plant's own Jacobians along the current trajectory, and whose line search, per-member
acceptance and convergence state run on the true plant without the iterate leaving the device.

The definition is here, in NumPy and SciPy.  Per member, with lo, hi the box with the du band on t = 0 as
plant_quad_program_reference builds them, J(X, U) = plant_linearize._objective and roll = T held-control plant steps from x0 under
u_scale * u:

    U = clip(U0, lo, hi);  X = roll(x0, U);  J = J(X, U);  cost_hist[0] = J
    if J not finite: status = 3, stop
    for i in 0 .. iters-1:
        U_qp = the U_opt of plant_quad_program_reference(X[:T], U, ..., x_init = x0, exact = exact)
        D = U_qp - U
        for j in 0 .. steps-1:  a_j = 2^-j;  U_j = clip(U + a_j D, lo, hi);  X_j = roll(x0, U_j);  J_j = J(X_j, U_j)
        j* = the smallest j attaining min_j J_j (a non-finite J_j is never chosen)
        if not J_j* < J: status = 2 (no descent: U, X, J kept), stop
        dec = J - J_j*;  J_old = J;  (U, X, J) = (U_j*, X_j*, J_j*);  alpha_hist[i] = a_j*;  cost_hist[i + 1] = J;  n_iter += 1
        if dec <= tol J_old: status = 1 (converged), stop
    status 0: the iterations are used up.  Unused alpha_hist entries are 0, unused cost_hist entries repeat the last J.

a_j is a power of two, so U + a_j D is one rounding (an fma on the device).  gains=True: one more linearisation and QP at the final
(X[:T], U), whatever the status; its gains are returned."""
from types import SimpleNamespace

import numpy as np

from . import _lib
from .feedback import _plant_step
from .plant_linearize import _clipped_member, _exact_member, _objective, _qp_common, _reference_points
from .rollout import _ptr

STATUS_ITERS, STATUS_CONVERGED, STATUS_NO_DESCENT, STATUS_NOT_FINITE = 0, 1, 2, 3
MAX_ITERS, MAX_STEPS = 64, 8


def _sqp_common(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind, u_scale):
    """Checks and lays out the arguments of plant_sqp_reference and plant_sqp_batch alike: what they share with
    plant_quad_program_batch goes through its _qp_common, with x0 repeated as the linearisation points."""
    x0 = np.asarray(x0)
    if x0.ndim != 2 or min(x0.shape) < 1:
        raise ValueError("x0 must be [B, n] (the initial states of B members), got shape %s" % (x0.shape,))
    x0 = np.ascontiguousarray(x0, dtype=np.complex128)
    B, n = x0.shape
    U0 = np.asarray(U0)
    if U0.ndim not in (2, 3) or min(U0.shape) < 1:
        raise ValueError("U0 must be [T, m] (shared) or [B|1, T, m], got shape %s" % (U0.shape,))
    T = U0.shape[-2]
    if isinstance(iters, bool) or isinstance(steps, bool) or int(iters) != iters or int(steps) != steps:
        raise TypeError("iters and steps must be integers, got %r and %r" % (iters, steps))
    iters, steps = int(iters), int(steps)
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError("iters must be in 1..%d, got %d" % (MAX_ITERS, iters))
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError("steps must be in 1..%d, got %d" % (MAX_STEPS, steps))
    tol = float(tol)
    if not (tol >= 0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and not negative, got %r" % (tol,))
    X = np.broadcast_to(x0[:, None, :], (B, T, n))
    (_, U0, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev,
     x0) = _qp_common(X, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x0, kind, u_scale)
    return x0, U0, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev, iters, steps, tol


def _clip(U, lo, hi):
    return np.minimum(np.maximum(U, lo), hi)


def _descent_reference(candidate, x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind, u_scale,
                       exact, gains, trace):
    """The module's loop, member by member, on plant_quad_program_reference's pieces and feedback._plant_step: the one definition
    of plant_sqp_reference and plant_ilqr_reference - the first guess, the tie rule, the tol rule, the statuses, the histories and
    the gains' QP.  candidate(mem, a, X, U, U_qp, rows) -> (X_j, U_j, J_j) is the candidate of step length a at the iterate (X, U),
    given what the QP there returned; mem holds the member: T, n, m, exact, x0, Xb, Ub, lo, hi, step(x, u, t) (one plant step under
    u_scale * u), cost(X, U) and roll(U) -> (X, J)."""
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

        def step(x, u, t):
            return _plant_step(kind, x, sc * u, H0, Hs, dts[t])

        def cost(X, U):
            with np.errstate(all="ignore"):
                return _objective(X, U, Xb, Ub, Q_ls, R_ls)

        def roll(U):
            X = np.empty((T + 1, n), dtype=np.complex128)
            X[0] = x0[b]
            for t in range(T):
                X[t + 1] = step(X[t], U[t], t)
            return X, cost(X, U)

        def qp(X, U):
            A, Bm, D = _reference_points(X[None, :T], U[None], 1, sc[None], H0[None], Hs[None], 1, dts, kind)
            return solve(x0[b], Xb, Ub, Q_ls, R_ls, A[0], Bm[0], D[0], lo, hi)

        mem = SimpleNamespace(T=T, n=n, m=m, exact=exact, x0=x0[b], Xb=Xb, Ub=Ub, lo=lo, hi=hi, step=step, cost=cost, roll=roll)
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
                    Xj, Uj, Jj = candidate(mem, a, X, U, U_qp, rows)
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


def _descent_batch(entry, x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind, u_scale, exact,
                   gains):
    """plant_sqp_batch and plant_ilqr_batch: one staging of one argument list around the C entry point named `entry`."""
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
    call = getattr(_lib.lib(), entry)
    _lib.check(call(B, n, m, kind, T, _ptr(dts), _ptr(x0), _ptr(U0), u_per, _ptr(u_scale), _ptr(op0), _ptr(ops), per, int(flags),
                    float(sat), float(du if band else 0.0), _ptr(X_bm), _ptr(U_bm), bm_per, _ptr(Q_ls), _ptr(R_ls), _ptr(u_prev), iters,
                    steps, tol, _ptr(out["X"]), _ptr(out["U"]), _ptr(out["cost"]), _ptr(out["cost_hist"]), _ptr(out["alpha_hist"]),
                    ip(out["n_iter"]), ip(out["status"]), _ptr(out["gains"])))
    return out


def _on_the_line(mem, a, X, U, U_qp, rows):
    """The SQP's candidate: the point clip(U + a (U_qp - U)) of the line to the QP's optimum, rolled in open loop."""
    Uj = _clip(U + a * (U_qp - U), mem.lo, mem.hi)
    Xj, Jj = mem.roll(Uj)
    return Xj, Uj, Jj


def plant_sqp_reference(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                        kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False, trace=None):
    """The definition of plant_sqp_batch (same arguments), on the host: the module's loop, member by member, on
    plant_quad_program_reference's pieces and feedback._plant_step.  trace: a list that receives one dict per (member, iteration) -
    "b", "i", "J" and "U" (the cost and the controls before), "U_qp", "Js" and "Us" (the candidates' costs and controls): what the decisions were taken on."""
    return _descent_reference(_on_the_line, x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, kind,
                              u_scale, exact, gains, trace)


def plant_sqp_batch(x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None,
                    kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=False):
    """A Gauss-Newton SQP on the plant's own dynamics for B members in ONE device call (m4q_plant_sqp_batch): up to `iters` times
    the QP of plant_quad_program_batch on the Jacobians along the member's current trajectory, a line search over the `steps` step
    lengths 1, 1/2, ... on the true plant, acceptance and convergence per member; the iterate stays on the device in between.

    x0 [B, n] complex: the initial states; U0 [T, m] (shared) or [B|1, T, m] real: the first guess (clipped into the bounds);
    op0, ops, dt_or_ts, kind, u_scale: the plant, as plant_linearize_batch; X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, exact: the
    cost and the bounds, as plant_quad_program_batch; iters in 1..64, steps in 1..8, tol >= 0: a member stops as converged when an
    accepted step lowers its cost by no more than tol times the cost.  Returns a dict: "X" [B, T + 1, n], "U" [B, T, m], "cost" [B],
    "cost_hist" [B, iters + 1], "alpha_hist" [B, iters], "n_iter" [B] and "status" [B] int32 (0 iterations used up, 1 converged,
    2 no candidate lowered the cost, 3 the first cost was not finite), "gains" [B, T, n + 1, m] (the QP's at the returned point) or
    None."""
    return _descent_batch("m4q_plant_sqp_batch", x0, U0, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev,
                          kind, u_scale, exact, gains)

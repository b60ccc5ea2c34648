"""The plant's own discrete-time Jacobians along trajectories, for whole ensembles in ONE launch (m4q_plant_linearize_batch): where
WrapModel.linearize_batch linearises a model - a truncated discretisation, or a fit - this linearises the held-control step of the
two unitary device plants itself, exactly.

The definition is here, in NumPy and SciPy.  Member b at point t is in state x = X[b, t] under the controls u = U[b|., t]; it sees
v_k = u_scale[b, k] u_k over the step length dts[t].  With X_e = -i dt (H0 + sum_k v_k H_k), E_k = -i dt H_k and
U, dU_k = grad._block_expm(X_e, E) (U = expm(X_e) and its Frechet derivatives, from one exponential of the (1 + m) d block matrix),
cols = 1 (Hamiltonian plant, n = d^2) or d^2 (process plant, n = d^4) and R = x.reshape(d, d, cols):
    A       = kron(kron(U, conj U), I_cols)                      [n, n]: it does not depend on the state
    B[:, k] = u_scale[b, k] vec(dU_k R U^H + U R dU_k^H)         the derivative with respect to the UNSCALED control u_k
    Delta   = -sum_k B[:, k] u_k, summed with k ascending from 0
The step is linear in the state, f(x, u) = A x, so A x + B u + Delta = f(x, u) to rounding, and the remainder of the expansion
around (x, u) is of second order in (dx, du).

Layouts are WrapModel.linearize_batch's: A [B, T, n, n], B [B, T, n, m], Delta [B, T, n], all complex, and go into
quad_program_batch unchanged.  Every shape is checked, and ValueError or TypeError raised, before the library is touched.  The
generator plant has no kernel (grad.py gives the reason): linearise its discretised model instead.

plant_quad_program_batch (m4q_plant_quad_program_batch) is plant_linearize_batch followed by quad_program_batch in ONE device call:
A is fully described by the d x d propagator U, so the call keeps U, B and Delta in device workspaces and the QP kernel forms the
entries of A it needs from U.  plant_quad_program_reference is its definition, in NumPy and SciPy."""
import numpy as np

from . import _lib
from .grad import _block_expm
from .rollout import _plant_operators, _ptr, dts_of

OUTPUTS = ("A", "B", "Delta")


def _point(x, u, sc, H0, Hs, dt, kind):
    """(A, B, Delta) of one point: the module's definition, line by line."""
    m = u.shape[0]
    d = H0.shape[0]
    cols = 1 if kind == _lib.PLANT_HAMILTONIAN else d * d
    H = H0.astype(np.complex128)
    for k in range(m):
        H = H + (sc[k] * u[k]) * Hs[k]
    U, dUs = _block_expm(-1j * dt * H, [-1j * dt * Hs[k] for k in range(m)])
    A = np.kron(np.kron(U, U.conj()), np.identity(cols))
    R = x.reshape(d, d, cols)
    Bm = np.empty((x.shape[0], m), dtype=np.complex128)
    Delta = np.zeros(x.shape[0], dtype=np.complex128)
    for k in range(m):
        Bm[:, k] = sc[k] * (np.einsum('ac,cgx,eg->aex', dUs[k], R, U.conj()) + np.einsum('ac,cgx,eg->aex', U, R, dUs[k].conj())).reshape(-1)
        Delta = Delta - Bm[:, k] * u[k]
    return A, Bm, Delta


def _wanted(outputs):
    if isinstance(outputs, str) or not isinstance(outputs, (tuple, list)):
        raise TypeError('outputs must be a tuple of names out of "A", "B", "Delta", got %r' % (outputs,))
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError('outputs: %r is none of "A", "B", "Delta"' % (name,))
    if not outputs:
        raise ValueError("outputs is empty: nothing to return")
    return tuple(name in outputs for name in OUTPUTS)


def _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs):
    """Checks and lays out the arguments of the definition and of the device call alike."""
    want = _wanted(outputs)
    kind = int(kind)
    if kind == _lib.PLANT_GENERATOR:
        raise ValueError("the generator plant has no linearisation of its own on the device: discretise its generators "
                         "(discretize_homogeneous_batch) and linearise the model (WrapModel.linearize_batch)")
    X = np.asarray(X)
    if X.ndim != 3 or min(X.shape) < 1:
        raise ValueError("X must be [B, T, n] (the T linearisation points of B members), got shape %s" % (X.shape,))
    X = np.ascontiguousarray(X, dtype=np.complex128)
    B, T, n = X.shape
    U = np.asarray(U)
    if np.iscomplexobj(U):
        raise TypeError("U must be real")
    U = np.ascontiguousarray(U, dtype=np.float64)
    if U.ndim not in (2, 3) or U.shape[-2] != T or U.shape[-1] < 1 or (U.ndim == 3 and U.shape[0] not in (1, B)):
        raise ValueError("U must be [T, m] (shared) or [B|1, T, m] with B = %d, T = %d, got shape %s" % (B, T, U.shape))
    u_per = 1 if (U.ndim == 3 and U.shape[0] == B and B > 1) else 0
    m = U.shape[-1]
    if u_scale is not None:
        u_scale = np.ascontiguousarray(u_scale, dtype=np.float64)
        if u_scale.shape != (B, m):
            raise ValueError("u_scale must be [B, m] = (%d, %d), got %s" % (B, m, u_scale.shape))
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, T)
    return X, U, u_per, u_scale, op0, ops, per, dts, kind, want


def plant_linearize_reference(X, U, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, outputs=OUTPUTS):
    """The definition of plant_linearize_batch (same arguments), on the host: SciPy's expm of the block matrix, point by point."""
    X, U, u_per, u_scale, op0, ops, per, dts, kind, want = _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs)
    return tuple(a if w else None for a, w in zip(_reference_points(X, U, u_per, u_scale, op0, ops, per, dts, kind), want))


def _reference_points(X, U, u_per, u_scale, op0, ops, per, dts, kind):
    """(A, B, Delta) of every point, from the arguments as _lin_common lays them out."""
    B, T, n = X.shape
    m = U.shape[-1]
    k = op0.shape[-1]
    o0, ok, useq = op0.reshape(-1, k, k), ops.reshape(-1, m, k, k), U.reshape(-1, T, m)
    A = np.empty((B, T, n, n), dtype=np.complex128)
    Bm = np.empty((B, T, n, m), dtype=np.complex128)
    Delta = np.empty((B, T, n), dtype=np.complex128)
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        for t in range(T):
            A[b, t], Bm[b, t], Delta[b, t] = _point(X[b, t], useq[b if u_per else 0, t], sc, o0[b if per else 0], ok[b if per else 0],
                                                    dts[t], kind)
    return A, Bm, Delta


def plant_linearize_batch(X, U, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, outputs=OUTPUTS):
    """The exact Jacobians of the plant step at B T points in one launch.

    X [B, T, n] complex: the points; U [T, m] (shared) or [B|1, T, m] real: the controls as the caller passes them; op0, ops, kind as
    plant_rollout_batch (kind PLANT_HAMILTONIAN or PLANT_PROCESS: the generator plant is refused); dt_or_ts a scalar dt or a time
    grid of T + 1 points; u_scale [B, m]: member b sees u_scale[b] * u.  outputs: which of "A", "B", "Delta" to compute and copy back
    (A is 16 n^2 bytes per point and not always wanted).  Returns (A [B, T, n, n], B [B, T, n, m], Delta [B, T, n]), None for an
    output not asked for; what is returned does not depend on what else was asked for."""
    X, U, u_per, u_scale, op0, ops, per, dts, kind, want = _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs)
    B, T, n = X.shape
    m = U.shape[-1]
    A = np.empty((B, T, n, n), dtype=np.complex128) if want[0] else None
    Bm = np.empty((B, T, n, m), dtype=np.complex128) if want[1] else None
    Delta = np.empty((B, T, n), dtype=np.complex128) if want[2] else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_linearize_batch(B, n, m, kind, T, _ptr(dts), _ptr(X), _ptr(U), u_per, _ptr(u_scale), _ptr(op0), _ptr(ops), per,
                                           _ptr(A), _ptr(Bm), _ptr(Delta)))
    return A, Bm, Delta


# ---------------------------------------------------------------- the QP on the plant's own linearisation, in one call
def _qp_common(X, U, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, kind, u_scale):
    """Checks and lays out the arguments of plant_quad_program_reference and plant_quad_program_batch alike."""
    X, U, u_per, u_scale, op0, ops, per, dts, kind, _ = _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, OUTPUTS)
    B, T, n = X.shape
    m = U.shape[-1]
    if sat is None or not float(sat) > 0:
        raise ValueError("sat must be positive, got %r" % (sat,))
    X_bm = np.asarray(X_bm)
    U_bm = np.asarray(U_bm)
    if np.iscomplexobj(U_bm):
        raise TypeError("U_bm must be real")
    if X_bm.shape not in ((T + 1, n), (1, T + 1, n), (B, T + 1, n)) or U_bm.shape not in ((T, m), (1, T, m), (B, T, m)):
        raise ValueError("X_bm must be [T + 1, n] = (%d, %d) and U_bm [T, m] = (%d, %d), shared or with a leading B|1 (B = %d), got %s "
                         "and %s" % (T + 1, n, T, m, B, X_bm.shape, U_bm.shape))
    X_bm = X_bm.reshape((-1, T + 1, n))
    U_bm = U_bm.reshape((-1, T, m))
    bm_per = 1 if (B > 1 and (X_bm.shape[0] == B or U_bm.shape[0] == B)) else 0
    if bm_per:                                        # (the QP takes both per member or both shared)
        X_bm, U_bm = np.broadcast_to(X_bm, (B, T + 1, n)), np.broadcast_to(U_bm, (B, T, m))
    X_bm = np.ascontiguousarray(X_bm, dtype=np.complex128)
    U_bm = np.ascontiguousarray(U_bm, dtype=np.float64)
    Q_ls, R_ls = np.asarray(Q_ls, dtype=np.complex128), np.asarray(R_ls, dtype=np.complex128)
    if Q_ls.shape == (n, n):
        Q_ls = np.broadcast_to(Q_ls, (T + 1, n, n))
    if R_ls.shape == (m, m):
        R_ls = np.broadcast_to(R_ls, (T, m, m))
    if Q_ls.shape != (T + 1, n, n) or R_ls.shape != (T, m, m):
        raise ValueError("Q_ls must be [T + 1, n, n] or [n, n] and R_ls [T, m, m] or [m, m], got %s and %s" % (Q_ls.shape, R_ls.shape))
    Q_ls, R_ls = np.ascontiguousarray(Q_ls), np.ascontiguousarray(R_ls)
    band = u_prev is not None and du is not None
    if band:
        u_prev = np.asarray(u_prev)
        if np.iscomplexobj(u_prev):
            raise TypeError("u_prev must be real")
        if u_prev.shape not in ((m,), (B, m)):
            raise ValueError("u_prev must be [m] or [B, m] = (%d, %d), got %s" % (B, m, u_prev.shape))
        u_prev = np.ascontiguousarray(np.broadcast_to(u_prev, (B, m)), dtype=np.float64)
        if not float(du) > 0:
            raise ValueError("du must be positive, got %r" % (du,))
    else:
        u_prev = None
    if x_init is not None:
        x_init = np.ascontiguousarray(x_init, dtype=np.complex128)
        if x_init.shape != (B, n):
            raise ValueError("x_init must be [B, n] = (%d, %d), got %s" % (B, n, x_init.shape))
    return X, U, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev, x_init


def _dag(M):
    return M.conj().T


def _sweep(Xb, Ub, Q, R, A, Bm, D, lo, hi, stat):
    """The affine Riccati sweep on z = [x - xbar; 1] of one member; returns the rows [T, m, n + 1].  stat None: every control free
    (the clipped mode's sweep).  stat [T, m] (0 free, +1 / -1 pinned on the upper / lower bound): the controls of the working set
    are constants of their stage, K row [0 | bound - ubar], the free ones respond to them, and what is returned in a pinned
    control's slot is the affine form of its multiplier, (H + G K) row k: the gradient of the stage with respect to u_k."""
    T, m = Ub.shape
    n = Xb.shape[1]

    def q_aug(Qt):
        out = np.zeros((n + 1, n + 1), dtype=complex)
        out[:n, :n] = Qt
        return out

    V = q_aug(Q[T])
    rows = np.empty((T, m, n + 1), dtype=complex)
    for t in reversed(range(T)):
        c = A[t] @ Xb[t] + Bm[t] @ Ub[t] + D[t] - Xb[t + 1]
        A_aug = np.block([[A[t], c.reshape(-1, 1)], [np.zeros((1, n)), np.ones((1, 1))]])
        B_aug = np.vstack([Bm[t], np.zeros((1, m))])
        G = R[t] + _dag(B_aug) @ V @ B_aug
        H = _dag(B_aug) @ V @ A_aug
        if stat is None:
            K = -np.linalg.pinv(G) @ H
            rows[t] = K
        else:
            p = stat[t] != 0
            f = ~p
            K = np.zeros((m, n + 1), dtype=complex)
            K[p, n] = (np.where(stat[t] > 0, hi[t], lo[t]) - Ub[t])[p]
            if f.any():
                K[f] = -np.linalg.solve(G[np.ix_(f, f)], H[f] + G[np.ix_(f, p)] @ K[p])
            rows[t] = np.where(p[:, None], H + G @ K, K)
        S = A_aug + B_aug @ K
        V = q_aug(Q[t]) + _dag(K) @ R[t] @ K + _dag(S) @ V @ S
    return rows


def _objective(X, U, Xb, Ub, Q, R):
    T = U.shape[0]
    cost = 0.0
    for t in range(T):
        ex, eu = X[t] - Xb[t], U[t] - Ub[t]
        cost += (ex.conj() @ Q[t] @ ex).real + (eu @ R[t] @ eu).real
    ex = X[T] - Xb[T]
    return float(cost + (ex.conj() @ Q[T] @ ex).real)


def _clipped_member(x0, Xb, Ub, Q, R, A, Bm, D, lo, hi):
    """The clipped QP of one member: the sweep, then the rollout of its policy with every control clipped into [lo, hi]."""
    T, m = Ub.shape
    rows = _sweep(Xb, Ub, Q, R, A, Bm, D, lo, hi, None)
    X = np.zeros((T + 1, Xb.shape[1]), dtype=complex)
    U = np.zeros((T, m))
    X[0] = x0
    for t in range(T):
        z = np.concatenate([X[t] - Xb[t], [1.0]])
        U[t] = np.minimum(np.maximum((rows[t] @ z).real + Ub[t], lo[t]), hi[t])
        X[t + 1] = A[t] @ X[t] + Bm[t] @ U[t] + D[t]
    return X, U, _objective(X, U, Xb, Ub, Q, R), rows


def _exact_member(x0, Xb, Ub, Q, R, A, Bm, D, lo, hi):
    """The box-constrained QP of one member solved exactly: the states condensed out, the bounded least-squares problem in the
    controls by SciPy's BVLS; the rows are those of the sweep with the controls on a bound at the optimum pinned (_sweep)."""
    from scipy.linalg import sqrtm
    from scipy.optimize import lsq_linear
    T, m = Ub.shape
    n = Xb.shape[1]

    def c2r(M):
        return np.block([[M.real, -M.imag], [M.imag, M.real]])

    def v2r(v):
        return np.concatenate([v.real, v.imag])

    free = [np.asarray(x0, dtype=complex)]
    for t in range(T):
        free.append(A[t] @ free[-1] + D[t])
    Phi = np.zeros((T + 1, n, T * m), dtype=complex)
    for s in range(T):
        for k in range(m):
            v = Bm[s][:, k]
            Phi[s + 1, :, s * m + k] = v
            for t in range(s + 1, T):
                v = A[t] @ v
                Phi[t + 1, :, s * m + k] = v
    rows_, rhs = [], []
    for t in range(T + 1):
        Wq = np.real(sqrtm(c2r(Q[t])))
        rows_.append(Wq @ np.vstack([Phi[t].real, Phi[t].imag]))
        rhs.append(Wq @ (v2r(Xb[t]) - v2r(free[t])))
    for t in range(T):
        Wr = np.real(sqrtm(R[t].real))
        E = np.zeros((m, T * m))
        E[:, t * m:(t + 1) * m] = np.identity(m)
        rows_.append(Wr @ E)
        rhs.append(Wr @ Ub[t])
    res = lsq_linear(np.vstack(rows_), np.concatenate(rhs), bounds=(lo.reshape(-1), hi.reshape(-1)), method='bvls', tol=1e-15,
                     max_iter=5000)
    U = res.x.reshape(T, m)
    X = np.zeros((T + 1, n), dtype=complex)
    X[0] = free[0]
    for t in range(T):
        X[t + 1] = A[t] @ X[t] + Bm[t] @ U[t] + D[t]
    stat = np.where(U >= hi, 1.0, np.where(U <= lo, -1.0, 0.0))
    return X, U, _objective(X, U, Xb, Ub, Q, R), _sweep(Xb, Ub, Q, R, A, Bm, D, lo, hi, stat)


def plant_quad_program_reference(X, U, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du=None, u_prev=None, x_init=None,
                                 kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=True):
    """The definition of plant_quad_program_batch (same arguments), on the host: plant_linearize_reference, then member by member the
    QP of optimize.quad_program on those Jacobians,
        min sum_t<T (x_t - xb_t)^H Q_t (x_t - xb_t) + (u_t - ub_t)^T R_t (u_t - ub_t) + (x_T - xb_T)^H Q_T (x_T - xb_T)
        x_{t+1} = A_t x_t + B_t u_t + Delta_t,  x_0 = x_init,  |u_t| <= sat,  |u_0 - u_prev| <= du,
    by the affine Riccati sweep with the bounds enforced by clipping in the rollout, or - exact - to the box-constrained optimum
    (BVLS on the condensed problem).  The gains [B, T, n + 1, m] are the sweep's rows, gains[b, t, :, k] acting on [x_t - xb_t; 1];
    exact: the rows of the sweep with the optimum's active controls pinned, a pinned control's slot holding its multiplier row (as
    quad_program_batch)."""
    (X, U, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev,
     x_init) = _qp_common(X, U, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, kind, u_scale)
    B, T, n = X.shape
    m = U.shape[-1]
    A, Bm, D = _reference_points(X, U, u_per, u_scale, op0, ops, per, dts, kind)
    X_opt = np.empty((B, T + 1, n), dtype=np.complex128)
    U_opt = np.empty((B, T, m), dtype=np.float64)
    cost = np.empty(B, dtype=np.float64)
    out = np.empty((B, T, n + 1, m), dtype=np.complex128)
    for b in range(B):
        lo, hi = np.full((T, m), -float(sat)), np.full((T, m), float(sat))
        if band:
            lo[0], hi[0] = np.maximum(lo[0], u_prev[b] - du), np.minimum(hi[0], u_prev[b] + du)
        x0 = X[b, 0] if x_init is None else x_init[b]
        solve = _exact_member if exact else _clipped_member
        X_opt[b], U_opt[b], cost[b], rows = solve(x0, X_bm[b if bm_per else 0], U_bm[b if bm_per else 0], Q_ls, R_ls, A[b], Bm[b], D[b],
                                                  lo, hi)
        out[b] = rows.transpose(0, 2, 1)
    return X_opt, U_opt, cost, (out if gains else None)


def plant_quad_program_batch(X, U, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du=None, u_prev=None, x_init=None,
                             kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False, gains=True):
    """quad_program_batch on the plant's own Jacobians along X, U, in ONE device call (m4q_plant_quad_program_batch): what
    plant_linearize_batch followed by quad_program_batch gives, without A, B and Delta crossing the host in between.

    X [B, T, n], U, op0, ops, dt_or_ts, kind, u_scale: the linearisation points and the plant, as plant_linearize_batch.  X_bm
    [T + 1, n] and U_bm [T, m], shared or with a leading B: the targets; Q_ls [T + 1, n, n] or [n, n], R_ls [T, m, m] or [m, m];
    sat, du and u_prev ([m] or [B, m]; the band needs both), exact: as quad_program_batch.  x_init [B, n]: the initial states,
    X[:, 0] when None.  gains=False skips the copy of the gains.  Returns (X_opt [B, T + 1, n], U_opt [B, T, m], cost [B],
    gains [B, T, n + 1, m] or None)."""
    (X, U, u_per, u_scale, op0, ops, per, dts, kind, X_bm, U_bm, bm_per, Q_ls, R_ls, band, u_prev,
     x_init) = _qp_common(X, U, op0, ops, dt_or_ts, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, kind, u_scale)
    B, T, n = X.shape
    m = U.shape[-1]
    flags = (_lib.QP_DU_BAND if band else 0) | (_lib.QP_EXACT_BOX if exact else 0)
    X_opt = np.empty((B, T + 1, n), dtype=np.complex128)
    U_opt = np.empty((B, T, m), dtype=np.float64)
    cost = np.empty(B, dtype=np.float64)
    out = np.empty((B, T, n + 1, m), dtype=np.complex128) if gains else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_quad_program_batch(B, n, m, kind, T, _ptr(dts), _ptr(X), _ptr(U), u_per, _ptr(u_scale), _ptr(op0), _ptr(ops), per,
                                              int(flags), float(sat), float(du if band else 0.0), _ptr(x_init), _ptr(X_bm), _ptr(U_bm),
                                              bm_per, _ptr(Q_ls), _ptr(R_ls), _ptr(u_prev), _ptr(X_opt), _ptr(U_opt), _ptr(cost), _ptr(out)))
    return X_opt, U_opt, cost, out

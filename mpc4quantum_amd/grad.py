"""Control gradients of open-loop rollouts for whole ensembles in ONE launch (m4q_plant_rollout_grad_batch,
m4q_model_rollout_grad_batch): what a pulse polished against an ensemble (robust GRAPE) needs - dJ_b/du[t][k] for every member, or
its weighted mean over the ensemble, and dJ_b/d u_scale[b][k], the sensitivity to a drive miscalibration.

The definitions are here, in NumPy and SciPy, in the kernels' order of operations.  Member b sees v[t][k] = u_scale[b][k] u[t][k];
the states x_0 .. x_N come from the rollouts' own step.  With d_t = x_t - f the figure is q_t = Re(d_t^H W d_t) (W [n, n] need not
be Hermitian), S = W + W^H and g_t = S d_t, so that dq_t = Re(g_t^H dx_t).  Two objectives: "last", J = q_N, and "sum",
J = sum_{t = 0..N} q_t.  The adjoint pass starts with lam_N = g_N and for t = N - 1 down to 0 forms
    ge[t][k] = Re(lam_{t+1}^H dx_{t+1}/dv_k),    lam_t = (dx_{t+1}/dx_t)^H lam_{t+1}  (+ g_t for "sum").
Outputs: grad[b][t][k] = u_scale[b][k] ge[t][k] (the derivative with respect to the unscaled sequence the caller passed) and
grad_scale[b][k] = sum_t u[t][k] ge[t][k], summed with t ascending.

Per step, Hamiltonian plant (n = d^2): X = -i dts[t] (H0 + sum_k v_k H_k), U = expm(X), dU_k = L(X, -i dts[t] H_k) its Frechet
derivative; dx_{t+1}/dv_k = vec_r(dU_k rho_t U^H + U rho_t dU_k^H) and lam_t = vec_r(U^H Lam_{t+1} U), Lam = mat(lam).  Process
plant (n = d^4): the same on every column of the d^2 x d^2 matrix M_t.  Model: dx_{t+1}/dv_k is column k of df_du at (x_t, v_t)
and lam_t = A(v_t)^H lam_{t+1}.  All Frechet derivatives of a step come from ONE matrix exponential of the (1 + m) d block matrix
with X on the diagonal blocks and [X, E_1 .. E_m] as its first block row: expm of it holds U in block (0, 0), dU_k in block (0, k).

Arrays keep the ensemble axis outermost, as the C ABI lays them out.  Every shape is checked, and ValueError raised, before the
library is touched."""
import numpy as np

from . import _lib
from .library import create_power_list, size_of_library
from .rollout import _common, _plant_operators, _ptr, dts_of

_FIGURES = {"last": 1, "sum": 2}
CHUNK = 256


# ---------------------------------------------------------------- the ensemble reduction
def ordered_weighted_sum(values, weights=None):
    """sum_b w_b values[b] over the leading axis in the order the device keeps: members in ascending chunks of 256, a sequential
    sum inside a chunk (from 0.0), then a sequential sum of the chunk partials (from 0.0); every product w_b * value is rounded
    before it is added.  w = weights [B], or 1 / B when absent.  Not NumPy's pairwise sum: the loops are explicit."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim < 1 or v.shape[0] < 1:
        raise ValueError("values must have a leading ensemble axis of at least one member, got shape %s" % (v.shape,))
    B = v.shape[0]
    if weights is None:
        w = np.full(B, 1.0 / B)
    else:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (B,):
            raise ValueError("weights must be [B] = (%d,), got %s" % (B, w.shape))
    total = np.zeros(v.shape[1:], dtype=np.float64)
    for c0 in range(0, B, CHUNK):
        part = np.zeros(v.shape[1:], dtype=np.float64)
        for b in range(c0, min(c0 + CHUNK, B)):
            part = part + w[b] * v[b]
        total = total + part
    return total


# ---------------------------------------------------------------- the definitions
def _figure_terms(x, W, S, f):
    d = x - f
    return float(np.real(d.conj() @ (W @ d))), S @ d


def _block_expm(X, Es):
    """U = expm(X) and the Frechet derivatives L(X, E_k), from one expm of the (1 + m) d block matrix."""
    from scipy.linalg import expm
    d, m = X.shape[0], len(Es)
    Z = np.zeros(((1 + m) * d, (1 + m) * d), dtype=np.complex128)
    for k in range(1 + m):
        Z[k * d:(k + 1) * d, k * d:(k + 1) * d] = X
    for k, E in enumerate(Es):
        Z[:d, (1 + k) * d:(2 + k) * d] = E
    F = expm(Z)
    return F[:d, :d], [F[:d, (1 + k) * d:(2 + k) * d] for k in range(m)]


def _finish(q_mode, qs, ge, u, sc):
    N, m = u.shape
    grad = sc[None, :] * ge
    gs = np.zeros(m)
    for t in range(N):
        gs = gs + u[t] * ge[t]
    return (qs if q_mode == 2 else qs[N]), grad, gs


def _plant_member(x0, u, sc, H0, Hs, dts, W, f, kind, q_mode):
    N, m = u.shape
    n = x0.shape[0]
    d = H0.shape[0]
    cols = 1 if kind == _lib.PLANT_HAMILTONIAN else d * d
    S = W + W.conj().T
    v = sc[None, :] * u

    def gens(t):
        H = H0.astype(np.complex128)
        for k in range(m):
            H = H + v[t, k] * Hs[k]
        return -1j * dts[t] * H, [-1j * dts[t] * Hs[k] for k in range(m)]

    # forward: rho+ = U rho U^H on every column of mat(x) [d, d, cols]
    xs = np.empty((N + 1, n), dtype=np.complex128)
    xs[0] = x0
    for t in range(N):
        X, Es = gens(t)
        U, _ = _block_expm(X, Es)
        R = xs[t].reshape(d, d, cols)
        xs[t + 1] = np.einsum('ac,cgx,eg->aex', U, R, U.conj()).reshape(-1)
    qs = np.empty(N + 1)
    gts = np.empty((N + 1, n), dtype=np.complex128)
    for t in range(N + 1):
        qs[t], gts[t] = _figure_terms(xs[t], W, S, f)
    ge = np.empty((N, m))
    lam = gts[N]
    for t in range(N - 1, -1, -1):
        X, Es = gens(t)
        U, dUs = _block_expm(X, Es)
        R = xs[t].reshape(d, d, cols)
        for k in range(m):
            dx = (np.einsum('ac,cgx,eg->aex', dUs[k], R, U.conj()) + np.einsum('ac,cgx,eg->aex', U, R, dUs[k].conj())).reshape(-1)
            ge[t, k] = np.real(lam.conj() @ dx)
        lam = np.einsum('ca,cgx,ge->aex', U.conj(), lam.reshape(d, d, cols), U).reshape(-1)
        if q_mode == 2:
            lam = lam + gts[t]
    return _finish(q_mode, qs, ge, u, sc)


def _model_member(x0, u, sc, model, powers, W, f, q_mode):
    N, m = u.shape
    n = x0.shape[0]
    P = len(powers)
    blocks = [model[:, p * n:(p + 1) * n] for p in range(1 + P)]
    S = W + W.conj().T
    v = sc[None, :] * u

    def mono(vt, e):
        out = 1.0
        for k in range(m):
            if e[k] < 0:
                return 0.0
            out = out * vt[k] ** int(e[k])
        return out

    def A_of(vt):
        A = blocks[0].astype(np.complex128)
        for p in range(P):
            A = A + mono(vt, powers[p]) * blocks[1 + p]
        return A

    xs = np.empty((N + 1, n), dtype=np.complex128)
    xs[0] = x0
    for t in range(N):
        xs[t + 1] = A_of(v[t]) @ xs[t]
    qs = np.empty(N + 1)
    gts = np.empty((N + 1, n), dtype=np.complex128)
    for t in range(N + 1):
        qs[t], gts[t] = _figure_terms(xs[t], W, S, f)
    ge = np.empty((N, m))
    lam = gts[N]
    unit = np.identity(m, dtype=int)
    for t in range(N - 1, -1, -1):
        for k in range(m):
            col = np.zeros(n, dtype=np.complex128)
            for p in range(P):
                if powers[p][k] > 0:
                    col = col + (powers[p][k] * mono(v[t], powers[p] - unit[k])) * (blocks[1 + p] @ xs[t])
            ge[t, k] = np.real(lam.conj() @ col)
        lam = A_of(v[t]).conj().T @ lam
        if q_mode == 2:
            lam = lam + gts[t]
    return _finish(q_mode, qs, ge, u, sc)


def _figure_mode(figure):
    if figure not in _FIGURES:
        raise ValueError('figure must be "last" (J = q_N) or "sum" (J = sum_t q_t), got %r' % (figure,))
    return _FIGURES[figure]


def _grad_common(x0, us, u_scale, W, target, figure, weights, reduce):
    """The rollouts' own checks and layout (rollout._common), and what the gradients add: the objective, the weights, reduce."""
    q_mode = _figure_mode(figure)
    if W is None or target is None:
        raise ValueError("the gradient needs W [n, n] and target [n] or [B, n]")
    x0, us, u_per, u_scale, W, target, t_per, _, _ = _common(x0, us, u_scale, W, target, "none", "last")
    B = x0.shape[0]
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (B,):
            raise ValueError("weights must be [B] = (%d,), got %s" % (B, weights.shape))
        if not np.all(np.isfinite(weights)) or np.any(weights < 0):
            raise ValueError("weights must be finite and non-negative")
    if reduce and u_per:
        raise ValueError("reduce=True needs one control sequence shared by the ensemble, got us %s" % (us.shape,))
    return x0, us, u_per, u_scale, W, target, t_per, q_mode, weights


def _models(models, order, B, n, m):
    order = int(order)
    if order < 1:
        raise ValueError("order must be at least 1, got %d" % order)
    P = size_of_library(order, m) - 1
    models = np.ascontiguousarray(models, dtype=np.complex128)
    if models.ndim not in (2, 3) or models.shape[-2:] != (n, n * (1 + P)) or (models.ndim == 3 and models.shape[0] not in (1, B)):
        raise ValueError("models must be [n, n (1 + P)] or [B|1, n, n (1 + P)] = (.., %d, %d) for order %d, m = %d, B = %d, got %s"
                         % (n, n * (1 + P), order, m, B, models.shape))
    return models, order, 1 if (models.ndim == 3 and models.shape[0] == B and B > 1) else 0


def _reference(member, x0, us, u_per, u_scale, target, t_per, q_mode, weights, reduce):
    B = x0.shape[0]
    N, m = us.shape[-2:]
    q = np.empty((B, N + 1) if q_mode == 2 else (B,))
    grad = np.empty((B, N, m))
    gs = np.empty((B, m))
    useq = us.reshape(-1, N, m)
    tg = target.reshape(-1, x0.shape[1])
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        q[b], grad[b], gs[b] = member(b, x0[b], useq[b if u_per else 0], sc, tg[b if t_per else 0])
    out = {"q": q, "grad": grad, "grad_scale": gs}
    if reduce:
        J = np.zeros(B)          # (a member's objective: its figures added with t ascending, as the device adds them)
        for t in range(N + 1 if q_mode == 2 else 1):
            J = J + (q[:, t] if q_mode == 2 else q)
        out["grad"] = ordered_weighted_sum(grad, weights)
        out["q_mean"] = float(ordered_weighted_sum(J, weights))
    return out


def plant_rollout_grad_reference(x0, us, op0, ops, dt_or_ts, W, target, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                                 weights=None, reduce=False):
    """The definition of plant_rollout_grad_batch (same arguments), on the host: returns "q", "grad", "grad_scale" and, with reduce,
    "q_mean".  SciPy's expm of the block matrix, member by member."""
    x0, us, u_per, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us, u_scale, W, target, figure, weights, reduce)
    B, n = x0.shape
    N, m = us.shape[-2:]
    if int(kind) == _lib.PLANT_GENERATOR:
        raise ValueError("the generator plant has no control gradient: take the gradient of its discretised model "
                         "(model_rollout_grad_reference)")
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, N)
    k = op0.shape[-1]
    o0, ok = op0.reshape(-1, k, k), ops.reshape(-1, m, k, k)
    return _reference(lambda b, x, u, sc, f: _plant_member(x, u, sc, o0[b if per else 0], ok[b if per else 0], dts, W, f, int(kind), q_mode),
                      x0, us, u_per, u_scale, target, t_per, q_mode, weights, reduce)


def model_rollout_grad_reference(x0, us, models, order, W, target, u_scale=None, figure="last", weights=None, reduce=False):
    """The definition of model_rollout_grad_batch (same arguments), on the host."""
    x0, us, u_per, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us, u_scale, W, target, figure, weights, reduce)
    B, n = x0.shape
    N, m = us.shape[-2:]
    models, order, m_per = _models(models, order, B, n, m)
    powers = create_power_list(order, m)[1:]
    md = models.reshape(-1, n, models.shape[-1])
    return _reference(lambda b, x, u, sc, f: _model_member(x, u, sc, md[b if m_per else 0], powers, W, f, q_mode),
                      x0, us, u_per, u_scale, target, t_per, q_mode, weights, reduce)


# ---------------------------------------------------------------- the device
def _grad_outputs(B, N, m, q_mode, reduce, scale_grad):
    q = np.empty((B, N + 1) if q_mode == 2 else (B,), dtype=np.float64)
    grad = np.empty((N, m) if reduce else (B, N, m), dtype=np.float64)
    gs = np.empty((B, m), dtype=np.float64) if scale_grad else None
    q_mean = np.empty(1, dtype=np.float64) if reduce else None
    return q, grad, gs, q_mean


def _grad_result(q, grad, gs, q_mean):
    out = {"q": q, "grad": grad}
    if gs is not None:
        out["grad_scale"] = gs
    if q_mean is not None:
        out["q_mean"] = float(q_mean[0])
    return out


def plant_rollout_grad_batch(x0, us, op0, ops, dt_or_ts, W, target, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                             weights=None, reduce=False, scale_grad=False):
    """The figure of an open-loop plant rollout and its gradient with respect to the controls, B members in one launch.

    x0, us, op0, ops, dt_or_ts, kind, u_scale, W, target as plant_rollout_batch (kind PLANT_HAMILTONIAN or PLANT_PROCESS: the
    generator plant is refused - dissipative dynamics go through model_rollout_grad_batch on the discretised model).
    figure: "last" -> J = q_N, q [B]; "sum" -> J = sum_t q_t, q [B, N + 1].  The q returned equals plant_rollout_batch's bit for bit.
    Returns a dict: "q"; "grad" [B, N, m] = dJ_b/du[t][k]; with scale_grad "grad_scale" [B, m] = dJ_b/du_scale[b][k];
    with reduce (one shared us) "grad" [N, m] = sum_b w_b grad[b] and "q_mean" = sum_b w_b J_b in the order of
    ordered_weighted_sum, w = weights [B] or 1 / B.  Without reduce, weights are checked and otherwise unused, as in the C ABI."""
    x0, us, u_per, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us, u_scale, W, target, figure, weights, reduce)
    B, n = x0.shape
    N, m = us.shape[-2:]
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, N)
    q, grad, gs, q_mean = _grad_outputs(B, N, m, q_mode, reduce, scale_grad)
    L = _lib.lib()
    _lib.check(L.m4q_plant_rollout_grad_batch(B, n, m, int(kind), N, _ptr(dts), _ptr(x0), _ptr(us), u_per, _ptr(u_scale), _ptr(op0),
                                              _ptr(ops), per, _ptr(W), _ptr(target), t_per, q_mode, _ptr(weights), 1 if reduce else 0,
                                              _ptr(q), _ptr(grad), _ptr(gs), _ptr(q_mean)))
    return _grad_result(q, grad, gs, q_mean)


def model_rollout_grad_batch(x0, us, models, order, W, target, u_scale=None, figure="last", weights=None, reduce=False,
                             scale_grad=False):
    """The figure of an open-loop model rollout (x+ = A [x ; lift_u(u) (x) x]) and its gradient with respect to the controls, B
    members in one launch.  x0, us, models, order, u_scale, W, target as model_rollout_batch; figure, weights, reduce, scale_grad
    and the returned dict as plant_rollout_grad_batch."""
    x0, us, u_per, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us, u_scale, W, target, figure, weights, reduce)
    B, n = x0.shape
    N, m = us.shape[-2:]
    models, order, m_per = _models(models, order, B, n, m)
    q, grad, gs, q_mean = _grad_outputs(B, N, m, q_mode, reduce, scale_grad)
    L = _lib.lib()
    _lib.check(L.m4q_model_rollout_grad_batch(B, n, m, order, N, _ptr(x0), _ptr(us), u_per, _ptr(u_scale), _ptr(models), m_per, _ptr(W),
                                              _ptr(target), t_per, q_mode, _ptr(weights), 1 if reduce else 0, _ptr(q), _ptr(grad),
                                              _ptr(gs), _ptr(q_mean)))
    return _grad_result(q, grad, gs, q_mean)

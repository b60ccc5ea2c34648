"""Plant-parameter gradients of open-loop rollouts and the per-member fit of plant parameters to measured trajectories
(m4q_plant_rollout_param_grad_batch): where the detunings, anharmonicities, crosstalk strengths and drive gains of an ensemble
come from.  Every designer of the package takes the members' op0 and u_scale as given; this module learns them from data, so that
the package runs measure -> calibrate -> design end to end.

The definitions are here, in NumPy and SciPy.  Member b's drift is op0_b + sum_j theta_j D_j with Hermitian directions D_j
(dirs), evaluated at the op0_b passed in - the gradient at the current point does not need the values of theta.  The states
x_0 .. x_N come from the rollouts' own step under v[t][k] = u_scale[b][k] u[t][k]; against the measured trajectory y = data the
objective is
    J_b = sum_t col_w[t] q_t,    q_t = Re((x_t - y_t)^H W (x_t - y_t)),
added with t ascending from 0.0, every product rounded before it is added; a column whose weight is 0 is skipped (sparse
measurement: what data holds there is never read).  With S = W + W^H and g_t = S (x_t - y_t) the adjoint pass starts from
lam_N = col_w[N] g_N and for t = N - 1 down to 0 forms
    grad_theta[j] += Re(lam_{t+1}^H dx_{t+1}/dtheta_j),    lam_t = (dx_{t+1}/dx_t)^H lam_{t+1} + col_w[t] g_t
(columns of weight 0 still propagate the costate).  Per step X = -i dts[t] (H0 + sum_k v_k H_k), U = expm(X) and
dU_j = L(X, E_j), the Frechet derivative in the direction E_j = -i dts[t] D_j; dx_{t+1}/dtheta_j = vec_r(dU_j rho_t U^H +
U rho_t dU_j^H), on every one of its d^2 columns for the process plant.  The drive gains are further directions of the same
construction: dJ/du_scale_k comes from E = -i dts[t] u[t][k] H_k, the derivative of X with respect to u_scale_k.  All
derivatives of a step come from ONE matrix exponential of the (1 + p_tot) d block matrix (grad._block_expm), which on the device
has to fit the 16 lanes of a row: p_tot = p + (m with scale_grad) <= 16 // d - 1.

The fit (plant_calibrate_reference, plant_calibrate_batch) is a projected L-BFGS per member over z_b = [theta_b, u_scale_b], written
once and vectorised over the members; calibrate_loop states it step by step.

Arrays keep the ensemble axis outermost, as the C ABI lays them out.  Every shape is checked, and ValueError raised, before the
library is touched."""
import numpy as np

from . import _lib
from .grad import _block_expm, _figure_terms
from .plant_robust import _int_in
from .rollout import _common, _plant_operators, _ptr, dts_of

STATUS_ITERS, STATUS_CONVERGED, STATUS_NO_DESCENT, STATUS_NOT_FINITE = 0, 1, 2, 3
MAX_ITERS, MAX_STEPS, MAX_MEM = 256, 16, 16
CURVATURE = 1e-12
HERMITIAN_TOL = 1e-12


# ---------------------------------------------------------------- arguments
def max_directions(d):
    """The largest p_tot a plant with d x d operators allows: the (1 + p_tot) d columns of the block matrix fit the 16 lanes of a row."""
    return 16 // int(d) - 1


def _param_common(x0, us, op0, ops, dirs, dt_or_ts, W, data, kind, u_scale, col_w, scale_grad):
    """The rollouts' own checks and layout, and what the parameter gradient adds: the directions, the data, the column weights."""
    if int(kind) == _lib.PLANT_GENERATOR:
        raise ValueError("the generator plant has no parameter gradient (its block matrix has (1 + p) n > 16 columns): fit the "
                         "parameters through its discretised model")
    if W is None or data is None or dirs is None:
        raise ValueError("the parameter gradient needs W [n, n], data [B|1, N + 1, n] and dirs [p, d, d]")
    x0 = np.ascontiguousarray(x0, dtype=np.complex128)
    n_guess = x0.shape[1] if x0.ndim == 2 and x0.shape[1] >= 1 else 1
    x0, us, u_per, u_scale, W, _, _, _, _ = _common(x0, us, u_scale, W, np.zeros(n_guess), "none", "last")
    B, n = x0.shape
    N, m = us.shape[-2:]
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    d = op0.shape[-1]
    dts = dts_of(dt_or_ts, N)
    dirs = np.ascontiguousarray(dirs, dtype=np.complex128)
    if dirs.ndim not in (3, 4) or dirs.shape[-2:] != (d, d) or dirs.shape[-3] < 1 or (dirs.ndim == 4 and dirs.shape[0] not in (1, B)):
        raise ValueError("dirs must be [p, d, d] or [B|1, p, d, d] with p >= 1, d = %d, B = %d, got %s" % (d, B, dirs.shape))
    p = dirs.shape[-3]
    scale = max(1.0, float(np.abs(dirs).max())) if dirs.size else 1.0
    if not np.all(np.isfinite(dirs)) or np.abs(dirs - np.conj(np.swapaxes(dirs, -1, -2))).max() > HERMITIAN_TOL * scale:
        raise ValueError("dirs must be finite Hermitian matrices (the drift op0 + sum_j theta_j D_j has to stay Hermitian)")
    p_tot = p + (m if scale_grad else 0)
    if p_tot > max_directions(d):
        raise ValueError("%d directions (p = %d%s) are too many for d = %d: the block matrix of (1 + p_tot) d columns must fit the 16 "
                         "lanes of a row, at most %d directions" % (p_tot, p, " and the m = %d drive gains" % m if scale_grad else "", d,
                                                                    max_directions(d)))
    d_per = 1 if (dirs.ndim == 4 and dirs.shape[0] == B and B > 1) else 0
    data = np.ascontiguousarray(data, dtype=np.complex128)
    if data.ndim not in (2, 3) or data.shape[-2:] != (N + 1, n) or (data.ndim == 3 and data.shape[0] not in (1, B)):
        raise ValueError("data must be [N + 1, n] or [B|1, N + 1, n] = (.., %d, %d), B = %d, got %s" % (N + 1, n, B, data.shape))
    y_per = 1 if (data.ndim == 3 and data.shape[0] == B and B > 1) else 0
    if col_w is None:
        col_w = np.ones(N + 1)
    col_w = np.ascontiguousarray(col_w, dtype=np.float64)
    if col_w.shape != (N + 1,):
        raise ValueError("col_w must be [N + 1] = (%d,), got %s" % (N + 1, col_w.shape))
    if not np.all(np.isfinite(col_w)) or np.any(col_w < 0):
        raise ValueError("col_w must be finite and non-negative")
    return x0, us, u_per, u_scale, op0, ops, per, dirs, d_per, dts, W, data, y_per, col_w


# ---------------------------------------------------------------- the definition
def _generator(t, v, H0, Hs, dts):
    H = H0.astype(np.complex128)
    for k in range(v.shape[1]):
        H = H + v[t, k] * Hs[k]
    return -1j * dts[t] * H


def member_states(x0, v, H0, Hs, dts, kind):
    """The definition's forward pass for one member under the controls v [N, m] it sees: xs [N + 1, n], rho+ = U rho U^H on every
    column of mat(x) [d, d, cols] (grad._plant_member's pass).  Data made by this from a member's true operators has J = 0 exactly
    at the truth."""
    N, n, d = v.shape[0], x0.shape[0], H0.shape[0]
    cols = 1 if int(kind) == _lib.PLANT_HAMILTONIAN else d * d
    xs = np.empty((N + 1, n), dtype=np.complex128)
    xs[0] = x0
    for t in range(N):
        U, _ = _block_expm(_generator(t, v, H0, Hs, dts), [])
        R = xs[t].reshape(d, d, cols)
        xs[t + 1] = np.einsum('ac,cgx,eg->aex', U, R, U.conj()).reshape(-1)
    return xs


def _param_member(x0, u, sc, H0, Hs, Ds, dts, W, y, cw, kind, scale_grad):
    N, m = u.shape
    n = x0.shape[0]
    d = H0.shape[0]
    p = len(Ds)
    cols = 1 if kind == _lib.PLANT_HAMILTONIAN else d * d
    S = W + W.conj().T
    v = sc[None, :] * u

    def gen(t):
        return _generator(t, v, H0, Hs, dts)

    xs = member_states(x0, v, H0, Hs, dts, kind)
    J = 0.0
    gts = np.zeros((N + 1, n), dtype=np.complex128)
    for t in range(N + 1):
        if cw[t] != 0.0:
            q, gts[t] = _figure_terms(xs[t], W, S, y[t])
            J = J + cw[t] * q
    g = np.zeros(p + (m if scale_grad else 0))
    lam = cw[N] * gts[N]
    for t in range(N - 1, -1, -1):
        Es = [-1j * dts[t] * Ds[j] for j in range(p)]
        if scale_grad:
            Es = Es + [-1j * dts[t] * u[t, k] * Hs[k] for k in range(m)]
        U, dUs = _block_expm(gen(t), Es)
        R = xs[t].reshape(d, d, cols)
        ge = np.empty(len(Es))
        for e, dU in enumerate(dUs):
            dx = (np.einsum('ac,cgx,eg->aex', dU, R, U.conj()) + np.einsum('ac,cgx,eg->aex', U, R, dU.conj())).reshape(-1)
            ge[e] = np.real(lam.conj() @ dx)
        g = g + ge
        lam = np.einsum('ca,cgx,ge->aex', U.conj(), lam.reshape(d, d, cols), U).reshape(-1)
        if cw[t] != 0.0:
            lam = lam + cw[t] * gts[t]
    return J, g[:p], g[p:]


def plant_param_grad_reference(x0, us, op0, ops, dirs, dt_or_ts, W, data, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, col_w=None,
                               scale_grad=False):
    """The definition of plant_rollout_param_grad_batch (same arguments), on the host: returns "J" [B], "grad_theta" [B, p] and, with
    scale_grad, "grad_scale" [B, m].  SciPy's expm of the block matrix, member by member."""
    x0, us, u_per, u_scale, op0, ops, per, dirs, d_per, dts, W, data, y_per, col_w = _param_common(
        x0, us, op0, ops, dirs, dt_or_ts, W, data, kind, u_scale, col_w, scale_grad)
    B, n = x0.shape
    N, m = us.shape[-2:]
    d, p = op0.shape[-1], dirs.shape[-3]
    o0, ok, dk = op0.reshape(-1, d, d), ops.reshape(-1, m, d, d), dirs.reshape(-1, p, d, d)
    useq, ys = us.reshape(-1, N, m), data.reshape(-1, N + 1, n)
    J, gt, gs = np.empty(B), np.empty((B, p)), np.empty((B, m))
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        J[b], gt[b], g_sc = _param_member(x0[b], useq[b if u_per else 0], sc, o0[b if per else 0], ok[b if per else 0],
                                          dk[b if d_per else 0], dts, W, ys[b if y_per else 0], col_w, int(kind), scale_grad)
        if scale_grad:
            gs[b] = g_sc
    out = {"J": J, "grad_theta": gt}
    if scale_grad:
        out["grad_scale"] = gs
    return out


# ---------------------------------------------------------------- the device
def plant_rollout_param_grad_batch(x0, us, op0, ops, dirs, dt_or_ts, W, data, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, col_w=None,
                                   scale_grad=False):
    """The misfit of an open-loop plant rollout against a measured trajectory and its gradient with respect to plant parameters, B
    members in one launch.

    x0, us, op0, ops, dt_or_ts, kind, u_scale, W as plant_rollout_grad_batch (kind PLANT_HAMILTONIAN or PLANT_PROCESS: the
    generator plant is refused); dirs [p, d, d] or [B|1, p, d, d]: Hermitian directions D_j, the member's drift being
    op0_b + sum_j theta_j D_j at the op0_b passed in; data [N + 1, n] or [B|1, N + 1, n]: the measured or wanted trajectory;
    col_w [N + 1] (default ones): non-negative column weights, zeros express sparse measurement.
    Returns a dict: "J" [B] = sum_t col_w[t] Re((x_t - y_t)^H W (x_t - y_t)), each figure plant_rollout_batch's own, added with t
    ascending; "grad_theta" [B, p] = dJ_b/dtheta_j; with scale_grad "grad_scale" [B, m] = dJ_b/du_scale[b][k].
    p + (m with scale_grad) <= 16 // d - 1 (7 at d = 2, 4 at d = 3, 3 at d = 4): more is a ValueError that names the limit."""
    x0, us, u_per, u_scale, op0, ops, per, dirs, d_per, dts, W, data, y_per, col_w = _param_common(
        x0, us, op0, ops, dirs, dt_or_ts, W, data, kind, u_scale, col_w, scale_grad)
    B, n = x0.shape
    N, m = us.shape[-2:]
    p = dirs.shape[-3]
    J, gt = np.empty(B, dtype=np.float64), np.empty((B, p), dtype=np.float64)
    gs = np.empty((B, m), dtype=np.float64) if scale_grad else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_rollout_param_grad_batch(B, n, m, int(kind), N, _ptr(dts), _ptr(x0), _ptr(us), u_per, _ptr(u_scale), _ptr(op0),
                                                    _ptr(ops), per, p, _ptr(dirs), d_per, _ptr(W), _ptr(data), y_per, _ptr(col_w),
                                                    _ptr(J), _ptr(gt), _ptr(gs)))
    out = {"J": J, "grad_theta": gt}
    if scale_grad:
        out["grad_scale"] = gs
    return out


# ---------------------------------------------------------------- the fit
def plant_param_op0(op0, dirs, theta):
    """op0_b + sum_j theta[b][j] D_j, added with j ascending: [B, d, d] from op0 [d, d] or [B|1, d, d], dirs [p, d, d] or
    [B|1, p, d, d] and theta [B, p].  The fit evaluates its iterates through this, and so should whoever makes data for it."""
    theta = np.asarray(theta, dtype=np.float64)
    B, p = theta.shape
    op0 = np.asarray(op0, dtype=np.complex128)
    dirs = np.asarray(dirs, dtype=np.complex128)
    d = op0.shape[-1]
    o0, dk = op0.reshape(-1, d, d), dirs.reshape(-1, p, d, d)
    if o0.shape[0] not in (1, B) or dk.shape[0] not in (1, B):
        raise ValueError("op0 [B|1, d, d] and dirs [B|1, p, d, d] must match theta [B, p] = %s, got %s and %s" % (theta.shape, op0.shape, dirs.shape))
    out = np.array(np.broadcast_to(o0, (B, d, d)))
    dk = np.broadcast_to(dk, (B, p, d, d))
    for j in range(p):
        out = out + theta[:, j, None, None] * dk[:, j]
    return np.ascontiguousarray(out)


def _steepest(pg, gmax, step0):
    safe = np.where(gmax > 0, gmax, 1.0)
    return -((step0 / safe)[:, None] * pg)


def _two_loop(Sm, Ym, cnt, pg):
    """r_b = H_b pg_b, H_b the L-BFGS inverse of member b's cnt[b] pairs (slot 0 oldest), scaled by (s.y) / (y.y) of its newest.
    Slots past cnt[b] hold nothing: their coefficients are 0.  Members without a pair get pg back."""
    B, mem, _ = Sm.shape
    v = pg.copy()
    valid = np.arange(mem)[None, :] < cnt[:, None]
    sy = np.sum(Sm * Ym, axis=2)
    rho = np.where(valid, 1.0 / np.where(valid, sy, 1.0), 0.0)
    a = np.zeros((B, mem))
    for k in range(mem - 1, -1, -1):
        a[:, k] = rho[:, k] * np.sum(Sm[:, k] * v, axis=1)
        v = v - a[:, k, None] * Ym[:, k]
    new = np.maximum(cnt - 1, 0)
    rows = np.arange(B)
    yy = np.sum(Ym[rows, new] * Ym[rows, new], axis=1)
    has = cnt > 0
    gamma = np.where(has, sy[rows, new] / np.where(has, yy, 1.0), 1.0)
    r = gamma[:, None] * v
    for k in range(mem):
        beta = rho[:, k] * np.sum(Ym[:, k] * r, axis=1)
        r = r + (a[:, k] - beta)[:, None] * Sm[:, k]
    return r


def calibrate_loop(z0, lo, hi, evaluate, iters=30, mem=5, steps=6, step0=0.1, tol=1e-12, gtol=1e-9, trace=None):
    """The fit's loop, once, vectorised over the members: a projected L-BFGS with a backtracking line search on
    evaluate(z [B, P]) -> (J [B], g [B, P]), lo <= z <= hi ([B, P], infinities allowed).  No member sees another's numbers: a member's
    run is the same whatever ensemble it is evaluated in.

        z = clip(z0);  (J, g) = evaluate(z);  cost_hist[b][:] = J_b;  J_b not finite: status 3
        iteration i = 0 .. iters-1, for every member still running:
          1. active = (z == lo and g > 0) or (z == hi and g < 0);  pg = g with active entries zeroed;  gmax = max |pg|;
             gmax <= gtol: status 1 (n_iter stays at the iterations begun before: a member that starts at a minimum stops with 0)
          2. n_iter = i + 1.  Empty memory: p = -(step0 / gmax) pg.  Otherwise the two-loop recursion on pg over the member's pairs,
             p = -r with active entries zeroed; not p.g < 0: the memory is cleared, p is the empty-memory direction
          3. candidates j = 0 .. steps-1 in turn: clip(z + 2^-j p); the first with a finite J_j < J is accepted (one evaluation
             of the ensemble per j, members that have decided ride along at the point they hold)
          4. accepted: s = z_j - z, y = g_j - g, kept as the newest pair if s.y > 1e-12 sqrt((s.s)(y.y)), the oldest beyond mem
             dropped; z = z_j, alpha_hist[i] = 2^-j, cost_hist[i+1:] = J_j;  J - J_j <= tol |J|: status 1
          5. not accepted: a non-empty memory is cleared and the next iteration tries the memoryless direction; an empty one: status 2
        status 0: the iterations are used up.  A member that has stopped keeps what it has.

    Returns a dict: "z" [B, P], "cost" [B], "cost_hist" [B, iters + 1], "alpha_hist" [B, iters], "n_iter" [B], "status" [B],
    "evaluations" (calls of evaluate).  trace: a list that receives one record per iteration."""
    z = np.clip(np.array(z0, dtype=np.float64), lo, hi)
    B, P = z.shape
    J, g = evaluate(z)
    J, g = np.array(J, dtype=np.float64), np.array(g, dtype=np.float64)
    evals = 1
    cost_hist = np.repeat(J[:, None], iters + 1, axis=1)
    alpha_hist = np.zeros((B, iters))
    n_iter, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    done = ~np.isfinite(J)
    status[done] = STATUS_NOT_FINITE
    Sm, Ym, cnt = np.zeros((B, max(mem, 1), P)), np.zeros((B, max(mem, 1), P)), np.zeros(B, dtype=np.int64)
    for i in range(iters):
        with np.errstate(all="ignore"):
            active = ((z == lo) & (g > 0)) | ((z == hi) & (g < 0))
            pg = np.where(active, 0.0, g)
            gmax = np.abs(pg).max(axis=1)
            conv = ~done & (gmax <= gtol)
            status[conv] = STATUS_CONVERGED
            done = done | conv
            live = ~done
            if not live.any():
                break
            n_iter[live] = i + 1
            p = _steepest(pg, gmax, step0)
            if mem > 0:
                q = np.where(active, 0.0, -_two_loop(Sm, Ym, cnt, pg))
                use = (cnt > 0) & (np.sum(q * g, axis=1) < 0)
                cnt = np.where((cnt > 0) & ~use, 0, cnt)
                p = np.where(use[:, None], q, p)
        acc = np.zeros(B, dtype=bool)
        z_new, J_new, g_new, alpha = z.copy(), J.copy(), g.copy(), np.zeros(B)
        for j in range(steps):
            need = live & ~acc
            if not need.any():
                break
            with np.errstate(all="ignore"):
                cand = np.where(need[:, None], np.clip(z + (2.0 ** -j) * p, lo, hi), z_new)
            Jc, gc = evaluate(cand)
            evals += 1
            Jc, gc = np.asarray(Jc, dtype=np.float64), np.asarray(gc, dtype=np.float64)
            with np.errstate(all="ignore"):
                ok = need & (Jc - Jc == 0.0) & (Jc < J)
            z_new[ok], J_new[ok], g_new[ok], alpha[ok] = cand[ok], Jc[ok], gc[ok], 2.0 ** -j
            acc = acc | ok
        if trace is not None:
            trace.append(dict(i=i, live=live.copy(), accepted=acc.copy(), alpha=alpha.copy(), z=z.copy(), J=J.copy(), p=p.copy()))
        with np.errstate(all="ignore"):
            s, y = z_new - z, g_new - g
            sy, ss, yy = np.sum(s * y, axis=1), np.sum(s * s, axis=1), np.sum(y * y, axis=1)
            keep = acc & (sy > CURVATURE * np.sqrt(ss * yy)) & (mem > 0)
            full = keep & (cnt == mem)
            Sm[full], Ym[full] = np.roll(Sm[full], -1, axis=1), np.roll(Ym[full], -1, axis=1)
            cnt = np.where(full, mem - 1, cnt)
            rows = np.nonzero(keep)[0]
            Sm[rows, cnt[rows]], Ym[rows, cnt[rows]] = s[rows], y[rows]
            cnt = np.where(keep, cnt + 1, cnt)
            conv = acc & (J - J_new <= tol * np.abs(J))
        cost_hist[acc, i + 1:] = J_new[acc, None]
        alpha_hist[:, i] = alpha
        z, J, g = z_new, J_new, g_new
        status[conv] = STATUS_CONVERGED
        done = done | conv
        rej = live & ~acc
        stuck = rej & (cnt == 0)
        status[stuck] = STATUS_NO_DESCENT
        done = done | stuck
        cnt = np.where(rej, 0, cnt)
    return {"z": z, "cost": J, "cost_hist": cost_hist, "alpha_hist": alpha_hist, "n_iter": n_iter, "status": status, "evaluations": evals}


def _calibrate(grad_fn, x0, us, op0, ops, dirs, dt_or_ts, W, data, theta0, bounds, fit_scale, u_scale, col_w, kind, iters, mem, steps,
               step0, tol, gtol, evaluate, trace):
    iters, steps, mem = _int_in("iters", iters, 1, MAX_ITERS), _int_in("steps", steps, 1, MAX_STEPS), _int_in("mem", mem, 0, MAX_MEM)
    step0, tol, gtol = float(step0), float(tol), float(gtol)
    if not (step0 > 0 and np.isfinite(step0)):
        raise ValueError("step0 must be positive and finite, got %r" % (step0,))
    if not (tol >= 0 and np.isfinite(tol)) or not (gtol >= 0 and np.isfinite(gtol)):
        raise ValueError("tol and gtol must be finite and not negative, got %r and %r" % (tol, gtol))
    x0c, usc, _, u_scale, op0c, _, _, dirsc, _, _, _, _, _, _ = _param_common(x0, us, op0, ops, dirs, dt_or_ts, W, data, kind, u_scale,
                                                                             col_w, fit_scale)
    B, m, p = x0c.shape[0], usc.shape[-1], dirsc.shape[-3]
    P = p + (m if fit_scale else 0)
    theta0 = np.zeros((B, p)) if theta0 is None else np.array(np.broadcast_to(np.asarray(theta0, dtype=np.float64), (B, p)))
    if not np.all(np.isfinite(theta0)):
        raise ValueError("theta0 must be finite")
    z0 = theta0
    if fit_scale:
        z0 = np.concatenate([theta0, np.ones((B, m)) if u_scale is None else u_scale], axis=1)
    if bounds is None:
        lo, hi = np.full((B, P), -np.inf), np.full((B, P), np.inf)
    else:
        try:
            lo, hi = (np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (B, P))) for v in bounds)
        except (TypeError, ValueError):
            raise ValueError("bounds must be a pair (lo, hi), each a scalar, [P] or [B, P] over the fitted [theta, u_scale], P = %d" % P)
        if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(lo > hi):
            raise ValueError("bounds: lo <= hi is required and neither may be NaN")

    def default_evaluate(z):
        sc = z[:, p:] if fit_scale else u_scale
        out = grad_fn(x0, us, plant_param_op0(op0c, dirsc, z[:, :p]), ops, dirs, dt_or_ts, W, data, kind=kind, u_scale=sc, col_w=col_w,
                      scale_grad=fit_scale)
        return out["J"], (np.concatenate([out["grad_theta"], out["grad_scale"]], axis=1) if fit_scale else out["grad_theta"])
    res = calibrate_loop(z0, lo, hi, default_evaluate if evaluate is None else evaluate, iters, mem, steps, step0, tol, gtol, trace)
    z = res.pop("z")
    out = {"theta": np.ascontiguousarray(z[:, :p])}
    if fit_scale:
        out["u_scale"] = np.ascontiguousarray(z[:, p:])
    out["op0"] = plant_param_op0(op0c, dirsc, z[:, :p])
    out.update(res)
    return out


def plant_calibrate_reference(x0, us, op0, ops, dirs, dt_or_ts, W, data, theta0=None, bounds=None, fit_scale=False, u_scale=None,
                              col_w=None, iters=30, mem=5, steps=6, tol=1e-12, gtol=1e-9, step0=0.1, kind=_lib.PLANT_HAMILTONIAN,
                              evaluate=None, trace=None):
    """The definition of plant_calibrate_batch (same arguments), on the host: calibrate_loop on plant_param_grad_reference.
    evaluate(z [B, P]) -> (J [B], g [B, P]) drives the same loop from any callable instead, z = [theta, u_scale]."""
    return _calibrate(plant_param_grad_reference, x0, us, op0, ops, dirs, dt_or_ts, W, data, theta0, bounds, fit_scale, u_scale, col_w,
                      kind, iters, mem, steps, step0, tol, gtol, evaluate, trace)


def plant_calibrate_batch(x0, us, op0, ops, dirs, dt_or_ts, W, data, theta0=None, bounds=None, fit_scale=False, u_scale=None,
                          col_w=None, iters=30, mem=5, steps=6, tol=1e-12, gtol=1e-9, step0=0.1, kind=_lib.PLANT_HAMILTONIAN, trace=None):
    """Fits plant parameters of B members to their measured trajectories: each member runs its own projected L-BFGS over theta_b
    (and, with fit_scale, its drive gains u_scale_b) on plant_rollout_param_grad_batch, one launch per evaluation for the whole
    ensemble (calibrate_loop states the loop).

    x0, us, op0, ops, dirs, dt_or_ts, W, data, col_w, kind, u_scale as plant_rollout_param_grad_batch; op0 is the nominal drift, the
    member's being op0_b + sum_j theta_j D_j.  theta0 [B, p] or [p] (default zeros) and u_scale (default ones) start the fit;
    bounds = (lo, hi), each a scalar, [P] or [B, P] over [theta, u_scale]; iters in 1..256, mem in 0..16 pairs, steps in 1..16
    candidates 2^-j per line search; step0 the largest entry of the first trial step of a memoryless direction; tol, gtol the
    relative-decrease and projected-gradient stops.
    Returns a dict: "theta" [B, p], "u_scale" [B, m] (with fit_scale), "op0" [B, d, d] at the result, "cost" [B], "cost_hist"
    [B, iters + 1], "alpha_hist" [B, iters], "n_iter" [B], "status" [B] (0 iterations used up, 1 converged, 2 no descent, 3 the
    first cost was not finite), "evaluations".
    The direction and the decision are taken on the host: per evaluation the loop itself moves 8 (p + m) bytes per member each way -
    the iterate up, the gradient (and J) down.  The one-shot entry restages the ensemble around them at every evaluation; keeping the
    ensemble, the iterate and the decision on the device is the follow-up."""
    return _calibrate(plant_rollout_param_grad_batch, x0, us, op0, ops, dirs, dt_or_ts, W, data, theta0, bounds, fit_scale, u_scale,
                      col_w, kind, iters, mem, steps, step0, tol, gtol, None, trace)

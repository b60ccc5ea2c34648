"""ONE pulse optimised against a whole ensemble (robust GRAPE) in one device call (m4q_plant_robust_batch), and the primitive its
line search runs on: S control sequences shared by the ensemble, each rolled against all B members in one launch
(m4q_plant_rollout_multi_batch).

Every other designer of the package returns a sequence per member - the best pulse if one knew which plant one holds.  Here the
objective is the weighted ensemble mean F(U) = sum_b w_b J_b(U) of plant_rollout_grad_batch(reduce=True), one U [N, m] for all
members, boxed to |u| <= sat.  The ensemble is staged once; an iteration is one reduced gradient (forward + adjoint pass) and one
launch that rolls all candidates of the line search forward; the direction and the decision are taken on the host between the
launches - they are one decision for the whole ensemble over N m numbers (the SQP's decisions are per member and stay on the device).

The definition is here, in NumPy, in the order of operations the C++ twin (csrc/m4q_robust_host.h) repeats: every dot product is
a sequential loop over (t, k) row-major from 0.0, every product is rounded before it is added.

    U = clip(U0);  memory = [] (at most mem pairs (s, y), newest last)
    iteration i = 0 .. iters-1:
      1. (F, g) = the reduced gradient at U (not taken again when U did not move).  i = 0: cost_hist[:] = F; F not finite: status 3
      2. active = (U == sat and g < 0) or (U == -sat and g > 0);  pg = g with active entries zeroed;  gmax = max |pg|;
         pgrad_hist[i] = gmax;  gmax <= gtol: status 1
      3. a pair pending from the last accepted step: y = g - g_old, kept if s.y > 1e-12 sqrt((s.s)(y.y)); the oldest beyond mem dropped
      4. empty memory: p = -(step0 / gmax) pg.  Otherwise the two-loop recursion on pg: newest to oldest rho = 1 / (s.y),
         a = rho (s.v), v -= a y; r = ((s.y) / (y.y))_newest v; oldest to newest r += (a - rho (y.r)) s; p = -r with active entries
         zeroed.  not p.g < 0 (a NaN too): the memory is cleared, p is the empty-memory direction
      5. candidates j = 0 .. steps-1: clip(U + 2^-j p) (2^-j p is exact; the clip lets a NaN through)
      6. F_j from the multi rollout; j* the smallest j attaining the least finite F_j; accepted if F_j* < F
      7. accepted: s = U_j* - U, g_old = g, U = U_j*, alpha_hist[i] = 2^-j*, cost_hist[i+1:] = F_j*;  F - F_j* <= tol |F|: status 1
      8. not accepted: a non-empty memory is cleared, alpha_hist[i] = 0, the next iteration reuses (F, g); an empty one: status 2
    status 0: the iterations are used up.  n_iter: the iterations begun (0 with status 3).  Unused cost_hist entries repeat the last
    cost, unused alpha_hist and pgrad_hist entries are 0.

Arrays keep the ensemble axis outermost.  Every shape is checked, and ValueError raised, before the library is touched."""
import numpy as np

from . import _lib
from .grad import _block_expm, _figure_terms, _grad_common, ordered_weighted_sum, plant_rollout_grad_reference
from .rollout import _plant_operators, _ptr, dts_of

STATUS_ITERS, STATUS_CONVERGED, STATUS_NO_DESCENT, STATUS_NOT_FINITE = 0, 1, 2, 3
MAX_ITERS, MAX_STEPS, MAX_MEM, MAX_S = 64, 8, 8, 8
CURVATURE = 1e-12


# ---------------------------------------------------------------- the direction (csrc/m4q_robust_host.h is its twin)
def _dot(a, b):
    """sum a[t][k] b[t][k], (t, k) row-major ascending from 0.0, every product rounded before it is added."""
    acc = 0.0
    for x, y in zip(np.ravel(a).tolist(), np.ravel(b).tolist()):
        acc = acc + x * y
    return acc


def _clip(w, sat):
    """min(max(w, -sat), sat) that lets a NaN through, as the device's clip does."""
    w = np.where(w < -sat, -sat, w)
    return np.where(w > sat, sat, w)


def _project(U, g, sat):
    """Step 2: (active, pg, gmax).  gmax is a sequential maximum of |pg| from 0.0 in which a NaN sticks."""
    active = ((U == sat) & (g < 0)) | ((U == -sat) & (g > 0))
    pg = np.where(active, 0.0, g)
    gmax = 0.0
    for v in np.ravel(pg).tolist():
        a = abs(v)
        if a > gmax or a != a:
            gmax = a
    return active, pg, gmax


def _absorb(pairs, s, g, g_old, mem):
    """Step 3: the pending pair (s, y = g - g_old) joins the memory if it passes the curvature test; the oldest beyond mem leaves."""
    y = g - g_old
    sy, ss, yy = _dot(s, y), _dot(s, s), _dot(y, y)
    if sy > CURVATURE * np.sqrt(ss * yy):
        pairs.append((s, y))
        while len(pairs) > mem:
            pairs.pop(0)


def _steepest(pg, gmax, step0):
    return -((step0 / gmax) * pg)


def _two_loop(pairs, pg):
    """r = H pg, H the L-BFGS inverse of the pairs (newest last) scaled by (s.y) / (y.y) of the newest."""
    v = pg.copy()
    coef = []
    for s, y in reversed(pairs):
        rho = 1.0 / _dot(s, y)
        a = rho * _dot(s, v)
        v = v - a * y
        coef.append((rho, a))
    s, y = pairs[-1]
    r = (_dot(s, y) / _dot(y, y)) * v
    for (s, y), (rho, a) in zip(pairs, reversed(coef)):
        r = r + (a - rho * _dot(y, r)) * s
    return r


def _direction(pairs, g, active, pg, gmax, step0):
    """Step 4.  May clear `pairs` (the quasi-Newton direction was not one of descent)."""
    if not pairs:
        return _steepest(pg, gmax, step0)
    p = np.where(active, 0.0, -_two_loop(pairs, pg))
    if not _dot(p, g) < 0:
        del pairs[:]
        return _steepest(pg, gmax, step0)
    return p


def _candidates(U, p, sat, steps):
    """Step 5: [steps, N, m]."""
    return np.stack([_clip(U + (2.0 ** -j) * p, sat) for j in range(steps)])


def _pick(Fs):
    """Step 6: the smallest j attaining the least finite F_j, or None."""
    best = None
    for j, Fj in enumerate(np.ravel(Fs).tolist()):
        if Fj - Fj == 0.0 and (best is None or Fj < Fs[best]):
            best = j
    return best


def _loop(U0, sat, iters, steps, mem, step0, tol, gtol, grad_fn, roll_fn, trace=None):
    """The module's loop on grad_fn(U [N, m]) -> (F, g [N, m]) and roll_fn(us [S, N, m]) -> F [S]."""
    U = _clip(np.array(U0, dtype=np.float64), sat)
    pairs, pending = [], None
    cost_hist, alpha_hist, pgrad_hist = np.zeros(iters + 1), np.zeros(iters), np.zeros(iters)
    status, n_iter, F, g, moved = STATUS_ITERS, 0, None, None, True
    for i in range(iters):
        if moved:
            F, g = grad_fn(U)
            F, g = float(F), np.asarray(g, dtype=np.float64)
            moved = False
            if i == 0:
                cost_hist[:] = F
                if not np.isfinite(F):
                    status = STATUS_NOT_FINITE
                    break
        n_iter = i + 1
        active, pg, gmax = _project(U, g, sat)
        pgrad_hist[i] = gmax
        if gmax <= gtol:
            status = STATUS_CONVERGED
            break
        if pending is not None:
            _absorb(pairs, pending[0], g, pending[1], mem)
            pending = None
        had = len(pairs)
        with np.errstate(all="ignore"):
            p = _direction(pairs, g, active, pg, gmax, step0)
            cands = _candidates(U, p, sat, steps)
        Fs = np.asarray(roll_fn(cands), dtype=np.float64)
        j = _pick(Fs)
        accepted = j is not None and Fs[j] < F
        if trace is not None:
            trace.append(dict(i=i, U=U, F=F, g=g, p=p, pairs=had, used=len(pairs), Fs=Fs, j=j if accepted else None))
        if accepted:
            pending, U, moved = (cands[j] - U, g), cands[j], True
            alpha_hist[i] = 2.0 ** -j
            cost_hist[i + 1:] = Fs[j]
            dec, F_old, F = F - Fs[j], F, float(Fs[j])
            if dec <= tol * abs(F_old):
                status = STATUS_CONVERGED
                break
        elif pairs:
            del pairs[:]
        else:
            status = STATUS_NO_DESCENT
            break
    return {"U": U, "cost": F, "cost_hist": cost_hist, "alpha_hist": alpha_hist, "pgrad_hist": pgrad_hist, "n_iter": n_iter,
            "status": status}


# ---------------------------------------------------------------- arguments
def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or int(v) != v:
        raise TypeError("%s must be an integer, got %r" % (name, v))
    if not lo <= int(v) <= hi:
        raise ValueError("%s must be in %d..%d, got %d" % (name, lo, hi, int(v)))
    return int(v)


def _robust_params(sat, iters, steps, mem, step0, tol, gtol):
    iters, steps, mem = _int_in("iters", iters, 1, MAX_ITERS), _int_in("steps", steps, 1, MAX_STEPS), _int_in("mem", mem, 0, MAX_MEM)
    sat, step0, tol, gtol = float(sat), float(step0), float(tol), float(gtol)
    if not sat > 0:
        raise ValueError("sat must be positive (inf: no box), got %r" % (sat,))
    if not (step0 > 0 and np.isfinite(step0)):
        raise ValueError("step0 must be positive and finite, got %r" % (step0,))
    if not (tol >= 0 and np.isfinite(tol)) or not (gtol >= 0 and np.isfinite(gtol)):
        raise ValueError("tol and gtol must be finite and not negative, got %r and %r" % (tol, gtol))
    return sat, iters, steps, mem, step0, tol, gtol


def _shared_sequence(U0, what):
    U0 = np.ascontiguousarray(U0, dtype=np.float64)
    if U0.ndim != 2 or min(U0.shape) < 1:
        raise ValueError("%s must be [N, m], one control sequence for the whole ensemble, got shape %s" % (what, U0.shape))
    return U0


def _no_generator(kind, who):
    if int(kind) == _lib.PLANT_GENERATOR:
        raise ValueError("%s: the generator plant has no control gradient - optimise on its discretised model "
                         "(model_rollout_grad_batch gives the gradient)" % who)


def _multi_common(x0, us, op0, ops, dt_or_ts, W, target, kind, u_scale, figure, weights):
    us = np.ascontiguousarray(us, dtype=np.float64)
    if us.ndim == 2:
        us = us[None]
    if us.ndim != 3 or min(us.shape) < 1:
        raise ValueError("us must be [S, N, m] (S sequences, each shared by the ensemble) or [N, m], got shape %s" % (us.shape,))
    if us.shape[0] > MAX_S:
        raise ValueError("us holds S = %d sequences, at most %d go into one launch" % (us.shape[0], MAX_S))
    x0, _, _, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us[0], u_scale, W, target, figure, weights, True)
    B, n = x0.shape
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, us.shape[2])
    return x0, us, u_scale, op0, ops, per, dts_of(dt_or_ts, us.shape[1]), W, target, t_per, q_mode, weights


# ---------------------------------------------------------------- the definitions
def _member_objective(x0, v, H0, Hs, dts, W, f, kind, q_mode):
    """J of one member under the controls v [N, m] it sees: grad._plant_member's forward pass and figures, statement for statement."""
    N, m = v.shape
    d = H0.shape[0]
    cols = 1 if kind == _lib.PLANT_HAMILTONIAN else d * d
    S = W + W.conj().T
    x = x0
    qs = np.empty(N + 1)
    qs[0], _ = _figure_terms(x, W, S, f)
    for t in range(N):
        H = H0.astype(np.complex128)
        for k in range(m):
            H = H + v[t, k] * Hs[k]
        U, _ = _block_expm(-1j * dts[t] * H, [-1j * dts[t] * Hs[k] for k in range(m)])
        x = np.einsum('ac,cgx,eg->aex', U, x.reshape(d, d, cols), U.conj()).reshape(-1)
        qs[t + 1], _ = _figure_terms(x, W, S, f)
    if q_mode != 2:
        return qs[N]
    J = 0.0
    for t in range(N + 1):
        J = J + qs[t]
    return J


def plant_rollout_multi_reference(x0, us, op0, ops, dt_or_ts, W, target, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                                  weights=None):
    """The definition of plant_rollout_multi_batch (same arguments), on the host: {"J": [B, S], "F": [S]}."""
    x0, us, u_scale, op0, ops, per, dts, W, target, t_per, q_mode, weights = _multi_common(x0, us, op0, ops, dt_or_ts, W, target, kind,
                                                                                           u_scale, figure, weights)
    _no_generator(kind, "plant_rollout_multi_reference")
    B, n = x0.shape
    S, N, m = us.shape
    k = op0.shape[-1]
    o0, ok, tg = op0.reshape(-1, k, k), ops.reshape(-1, m, k, k), target.reshape(-1, n)
    J = np.empty((B, S))
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        for s in range(S):
            J[b, s] = _member_objective(x0[b], sc[None, :] * us[s], o0[b if per else 0], ok[b if per else 0], dts, W,
                                        tg[b if t_per else 0], int(kind), q_mode)
    return {"J": J, "F": ordered_weighted_sum(J, weights)}


def plant_robust_reference(x0, U0, op0, ops, dt_or_ts, W, target, sat, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                           weights=None, iters=10, steps=6, mem=5, step0=0.1, tol=1e-9, gtol=0.0, members=False, evaluate=None,
                           trace=None):
    """The definition of plant_robust_batch (same arguments), on the host: the module's loop on plant_rollout_grad_reference and
    plant_rollout_multi_reference.  evaluate=(grad_fn, roll_fn) drives the same loop from any pair of callables instead:
    grad_fn(U [N, m]) -> (F, g [N, m]), roll_fn(us [S, N, m]) -> F [S] (then only U0 and the loop's parameters are read; with
    members, roll_fn(us, members=True) -> (F, J [B, S])).  trace: a list that receives one record per iteration."""
    sat, iters, steps, mem, step0, tol, gtol = _robust_params(sat, iters, steps, mem, step0, tol, gtol)
    U0 = _shared_sequence(U0, "U0")
    if evaluate is None:
        _no_generator(kind, "plant_robust_reference")
        args = (x0, op0, ops, dt_or_ts, W, target)
        kw = dict(kind=kind, u_scale=u_scale, figure=figure, weights=weights)
        _multi_common(x0, U0, op0, ops, dt_or_ts, W, target, kind, u_scale, figure, weights)

        def grad_fn(U):
            out = plant_rollout_grad_reference(args[0], U, *args[1:], reduce=True, **kw)
            return out["q_mean"], out["grad"]

        def roll_fn(us, members=False):
            out = plant_rollout_multi_reference(args[0], us, *args[1:], **kw)
            return (out["F"], out["J"]) if members else out["F"]
    else:
        grad_fn, roll_fn = evaluate
    out = _loop(U0, sat, iters, steps, mem, step0, tol, gtol, grad_fn, roll_fn, trace)
    if members:
        out["J"] = np.asarray(roll_fn(out["U"][None], members=True)[1], dtype=np.float64)[:, 0]
    return out


# ---------------------------------------------------------------- the device
def plant_rollout_multi_batch(x0, us, op0, ops, dt_or_ts, W, target, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                              weights=None, members=True, mean=True):
    """S control sequences, each shared by the ensemble, rolled against all B members in ONE launch: compare pulses, or scan an
    amplitude, over an ensemble.

    x0 [B, n]; us [S, N, m] (1 <= S <= 8) or [N, m]; op0, ops, dt_or_ts, kind, u_scale, W, target as plant_rollout_grad_batch (the
    generator plant is refused).  figure: "last" -> J = q_N, "sum" -> J = sum_t q_t.  Returns a dict: with members "J" [B, S], the
    members' objectives - J[:, s] has the bits of plant_rollout_batch's figure under us[s]; with mean "F" [S] = sum_b w_b J[b, s]
    in the order of ordered_weighted_sum, w = weights [B] or 1 / B."""
    x0, us, u_scale, op0, ops, per, dts, W, target, t_per, q_mode, weights = _multi_common(x0, us, op0, ops, dt_or_ts, W, target, kind,
                                                                                           u_scale, figure, weights)
    if not (members or mean):
        raise ValueError("members=False with mean=False: nothing to return")
    B, n = x0.shape
    S, N, m = us.shape
    J = np.empty((B, S), dtype=np.float64) if members else None
    F = np.empty(S, dtype=np.float64) if mean else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_rollout_multi_batch(B, n, m, int(kind), N, _ptr(dts), _ptr(x0), S, _ptr(us), _ptr(u_scale), _ptr(op0),
                                               _ptr(ops), per, _ptr(W), _ptr(target), t_per, q_mode, _ptr(weights), _ptr(J), _ptr(F)))
    out = {}
    if members:
        out["J"] = J
    if mean:
        out["F"] = F
    return out


def plant_robust_batch(x0, U0, op0, ops, dt_or_ts, W, target, sat, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, figure="last",
                       weights=None, iters=10, steps=6, mem=5, step0=0.1, tol=1e-9, gtol=0.0, members=False):
    """ONE control sequence optimised against the weighted mean of an ensemble, in one device call: a projected L-BFGS on
    F(U) = sum_b w_b J_b(U), |U| <= sat (the module's loop).

    x0 [B, n]; U0 [N, m], the first guess shared by the ensemble; op0, ops, dt_or_ts, kind, u_scale, W, target, figure, weights as
    plant_rollout_grad_batch(reduce=True) (the generator plant is refused); sat > 0 the box (inf: none); iters in 1..64; steps in
    1..8 candidates 2^-j per line search; mem in 0..8 pairs of the quasi-Newton memory (0: projected gradient); step0 the length
    of the largest entry of the first trial step of a memoryless direction; tol, gtol the relative-decrease and projected-gradient
    stops.  Returns a dict: "U" [N, m], "cost", "cost_hist" [iters + 1], "alpha_hist" [iters], "pgrad_hist" [iters], "n_iter",
    "status" (0 iterations used up, 1 converged, 2 no descent, 3 the first cost was not finite) and, with members, "J" [B], the
    members' objectives at U."""
    sat, iters, steps, mem, step0, tol, gtol = _robust_params(sat, iters, steps, mem, step0, tol, gtol)
    U0 = _shared_sequence(U0, "U0")
    x0, us, u_scale, op0, ops, per, dts, W, target, t_per, q_mode, weights = _multi_common(x0, U0, op0, ops, dt_or_ts, W, target, kind,
                                                                                           u_scale, figure, weights)
    B, n = x0.shape
    N, m = U0.shape
    U, cost = np.empty((N, m)), np.empty(1)
    cost_hist, alpha_hist, pgrad_hist = np.empty(iters + 1), np.empty(iters), np.empty(iters)
    n_iter, status = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    J = np.empty(B) if members else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_robust_batch(B, n, m, int(kind), N, _ptr(dts), _ptr(x0), _ptr(U0), _ptr(u_scale), _ptr(op0), _ptr(ops), per,
                                        _ptr(W), _ptr(target), t_per, q_mode, _ptr(weights), sat, iters, steps, mem, step0, tol, gtol,
                                        _ptr(U), _ptr(cost), _ptr(cost_hist), _ptr(alpha_hist), _ptr(pgrad_hist),
                                        n_iter.ctypes.data_as(_lib._ip), status.ctypes.data_as(_lib._ip), _ptr(J)))
    out = {"U": U, "cost": float(cost[0]), "cost_hist": cost_hist, "alpha_hist": alpha_hist, "pgrad_hist": pgrad_hist,
           "n_iter": int(n_iter[0]), "status": int(status[0])}
    if members:
        out["J"] = J
    return out

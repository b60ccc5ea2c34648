"""Open-loop rollouts: a known control sequence applied to a whole ensemble of plants or models in ONE launch
(m4q_plant_rollout_batch, m4q_model_rollout_batch) - `QExperiment.simulate` / `DMDc.predict` along a sequence for B members,
with the state kept in registers from x0 to the last step.

Arrays keep the ensemble axis outermost, as the C ABI lays them out: a trajectory is xs [B, N + 1, n] (column 0 = x0 as given),
a final state [B, n]; the figure q = Re((x - f)^H W (x - f)) is [B, N + 1] or [B].  Every shape is checked, and ValueError
raised, before the library is touched."""
import numpy as np

from . import _lib
from .library import size_of_library

_MODES = {"none": 0, "last": 1, "all": 2}


def dts_of(dt_or_ts, N):
    """The N held-control interval lengths: a scalar dt repeated, or the differences of a time grid ts of N + 1 points
    (which need not be uniform)."""
    t = np.asarray(dt_or_ts, dtype=np.float64)
    if t.ndim == 0:
        dts = np.full(N, float(t))
    elif t.ndim == 1 and t.shape[0] == N + 1:
        dts = np.diff(t)
    else:
        raise ValueError("dt_or_ts must be a scalar dt or a time grid of N + 1 = %d points, got shape %s" % (N + 1, t.shape))
    if not np.all(np.isfinite(dts)):
        raise ValueError("dt_or_ts: the interval lengths must be finite")
    return np.ascontiguousarray(dts)


def _plant_dim(kind, n):
    """Side k of the plant operators (HAMILTONIAN: n = k^2, PROCESS: n = k^4, GENERATOR: k = n)."""
    kind = int(kind)
    if kind == _lib.PLANT_GENERATOR:
        r = int(round(n ** 0.5))
        if r * r != n:
            raise ValueError("generator plant: n = %d is not a square (the state is a vectorised density matrix)" % n)
        return n
    if kind == _lib.PLANT_HAMILTONIAN:
        k = int(round(n ** 0.5))
        if k * k != n:
            raise ValueError("Hamiltonian plant: n = %d is not a square" % n)
        return k
    if kind == _lib.PLANT_PROCESS:
        k = int(round(n ** 0.25))
        if k ** 4 != n:
            raise ValueError("process plant: n = %d is not a fourth power" % n)
        return k
    raise ValueError("kind must be PLANT_HAMILTONIAN, PLANT_GENERATOR or PLANT_PROCESS, got %r" % (kind,))


def _common(x0, us, u_scale, W, target, keep, figure, need_output=True):
    """Checks and lays out what the two rollouts share.  Returns (x0, us, u_per, u_scale, W, target, t_per, xs_mode, q_mode).
    need_output: neither states nor figures is a refusal (the feedback runs, which return more, pass False)."""
    if keep not in _MODES or figure not in _MODES:
        raise ValueError('keep and figure must be "none", "last" or "all", got %r and %r' % (keep, figure))
    xs_mode, q_mode = _MODES[keep], _MODES[figure]
    if need_output and xs_mode == 0 and q_mode == 0:
        raise ValueError('keep="none" with figure="none": nothing to return')
    x0 = np.ascontiguousarray(x0, dtype=np.complex128)
    if x0.ndim != 2 or x0.shape[0] < 1 or x0.shape[1] < 1:
        raise ValueError("x0 must be [B, n], got shape %s" % (x0.shape,))
    B, n = x0.shape
    us = np.ascontiguousarray(us, dtype=np.float64)
    if us.ndim not in (2, 3) or us.shape[-2] < 1 or us.shape[-1] < 1:
        raise ValueError("us must be [N, m] (one sequence for the ensemble) or [B, N, m], got shape %s" % (us.shape,))
    if us.ndim == 3 and us.shape[0] not in (1, B):
        raise ValueError("us has %d sequences for %d members" % (us.shape[0], B))
    u_per = 1 if (us.ndim == 3 and us.shape[0] == B and B > 1) else 0
    N, m = us.shape[-2:]
    if u_scale is not None:
        u_scale = np.ascontiguousarray(u_scale, dtype=np.float64)
        if u_scale.shape != (B, m):
            raise ValueError("u_scale must be [B, m] = (%d, %d), got %s" % (B, m, u_scale.shape))
    t_per = 0
    if q_mode:
        if W is None or target is None:
            raise ValueError('figure="%s" needs W [n, n] and target [n] or [B, n]' % figure)
        W = np.ascontiguousarray(W, dtype=np.complex128)
        target = np.ascontiguousarray(target, dtype=np.complex128)
        if W.shape != (n, n):
            raise ValueError("W must be [n, n] = (%d, %d), got %s" % (n, n, W.shape))
        if target.shape not in ((n,), (1, n), (B, n)):
            raise ValueError("target must be [n] or [B, n] with n = %d, B = %d, got %s" % (n, B, target.shape))
        t_per = 1 if (target.ndim == 2 and target.shape[0] == B and B > 1) else 0
    else:
        W = target = None
    return x0, us, u_per, u_scale, W, target, t_per, xs_mode, q_mode


def _outputs(B, N, n, xs_mode, q_mode):
    xs = None if xs_mode == 0 else np.empty((B, N + 1, n) if xs_mode == 2 else (B, n), dtype=np.complex128)
    q = None if q_mode == 0 else np.empty((B, N + 1) if q_mode == 2 else (B,), dtype=np.float64)
    return xs, q


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_lib._dp)


def _result(xs, q):
    out = {}
    if xs is not None:
        out["xs"] = xs
    if q is not None:
        out["q"] = q
    return out


def _plant_operators(op0, ops, kind, B, n, m):
    """Checks and lays out the plant operators of B members: returns (op0, ops, per)."""
    k = _plant_dim(kind, n)
    op0 = np.ascontiguousarray(op0, dtype=np.complex128)
    ops = np.ascontiguousarray(ops, dtype=np.complex128)
    if op0.ndim not in (2, 3) or op0.shape[-2:] != (k, k) or (op0.ndim == 3 and op0.shape[0] not in (1, B)):
        raise ValueError("op0 must be [k, k] or [B|1, k, k] with k = %d, B = %d, got %s" % (k, B, op0.shape))
    if ops.ndim not in (3, 4) or ops.shape[-3:] != (m, k, k) or (ops.ndim == 4 and ops.shape[0] not in (1, B)):
        raise ValueError("ops must be [m, k, k] or [B|1, m, k, k] with m = %d, k = %d, B = %d, got %s" % (m, k, B, ops.shape))
    per0 = op0.ndim == 3 and op0.shape[0] == B and B > 1
    perk = ops.ndim == 4 and ops.shape[0] == B and B > 1
    per = 1 if (per0 or perk) else 0
    if per:          # the kernel reads both operator sets with the member's stride: repeat the shared one
        if not per0:
            op0 = np.ascontiguousarray(np.broadcast_to(op0.reshape(-1, k, k)[:1], (B, k, k)))
        if not perk:
            ops = np.ascontiguousarray(np.broadcast_to(ops.reshape(-1, m, k, k)[:1], (B, m, k, k)))
    return op0, ops, per


def plant_rollout_batch(x0, us, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, W=None, target=None, keep="all",
                        figure="none"):
    """N held-control plant steps of B members in one launch.

    x0 [B, n]; us [N, m] (shared) or [B, N, m]; op0 [k, k] or [B|1, k, k], ops [m, k, k] or [B|1, m, k, k] as plant_step_batch
    (k = d for HAMILTONIAN, n = d^2, and PROCESS, n = d^4; k = n for GENERATOR); dt_or_ts a scalar dt or a time grid of N + 1 points;
    u_scale [B, m]: member b is driven by u_scale[b] * us[t].
    keep: "all" -> xs [B, N + 1, n], "last" -> xs [B, n], "none".  figure: "all" -> q [B, N + 1], "last" -> q [B], "none";
    q = Re((x - target)^H W (x - target)) with W [n, n] and target [n] or [B, n].  Returns a dict with "xs" and / or "q"."""
    x0, us, u_per, u_scale, W, target, t_per, xs_mode, q_mode = _common(x0, us, u_scale, W, target, keep, figure)
    B, n = x0.shape
    N, m = us.shape[-2:]
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, N)
    xs, q = _outputs(B, N, n, xs_mode, q_mode)
    L = _lib.lib()
    _lib.check(L.m4q_plant_rollout_batch(B, n, m, int(kind), N, _ptr(dts), _ptr(x0), _ptr(us), u_per, _ptr(u_scale), _ptr(op0),
                                         _ptr(ops), per, _ptr(W), _ptr(target), t_per, xs_mode, _ptr(xs), q_mode, _ptr(q)))
    return _result(xs, q)


def model_rollout_batch(x0, us, models, order, u_scale=None, W=None, target=None, keep="all", figure="none"):
    """N model steps x+ = A [x ; lift_u(u) (x) x] (DMDc.predict with WrapModel's lifted controls) of B members in one launch.

    x0 [B, n]; us [N, m] or [B, N, m]; models [n, n (1 + P)] or [B|1, n, n (1 + P)] with P = size_of_library(order, m) - 1;
    u_scale, W, target, keep, figure and the returned dict as plant_rollout_batch."""
    x0, us, u_per, u_scale, W, target, t_per, xs_mode, q_mode = _common(x0, us, u_scale, W, target, keep, figure)
    B, n = x0.shape
    N, m = us.shape[-2:]
    order = int(order)
    if order < 1:
        raise ValueError("order must be at least 1, got %d" % order)
    P = size_of_library(order, m) - 1
    models = np.ascontiguousarray(models, dtype=np.complex128)
    if models.ndim not in (2, 3) or models.shape[-2:] != (n, n * (1 + P)) or (models.ndim == 3 and models.shape[0] not in (1, B)):
        raise ValueError("models must be [n, n (1 + P)] or [B|1, n, n (1 + P)] = (.., %d, %d) for order %d, m = %d, B = %d, got %s"
                         % (n, n * (1 + P), order, m, B, models.shape))
    m_per = 1 if (models.ndim == 3 and models.shape[0] == B and B > 1) else 0
    xs, q = _outputs(B, N, n, xs_mode, q_mode)
    L = _lib.lib()
    _lib.check(L.m4q_model_rollout_batch(B, n, m, order, N, _ptr(x0), _ptr(us), u_per, _ptr(u_scale), _ptr(models), m_per, _ptr(W),
                                         _ptr(target), t_per, xs_mode, _ptr(xs), q_mode, _ptr(q)))
    return _result(xs, q)


def held_controls(us, ts, m, B):
    """The controls of simulate() - a callable of time, or an array whose column i is held on [ts[i], ts[i + 1]) - as the
    rollouts take them: (m, >= N) -> [N, m], (B, m, >= N) -> [B, N, m]."""
    ts = np.asarray(ts, dtype=np.float64)
    if ts.ndim != 1 or ts.shape[0] < 2:
        raise ValueError("ts must be a time grid of at least two points, got shape %s" % (ts.shape,))
    N = ts.shape[0] - 1
    if callable(us):
        return np.stack([np.real(np.reshape(us(ts[i]), -1)[:m]) for i in range(N)]).astype(np.float64)
    us = np.asarray(us)
    if us.ndim == 1:
        us = us[None]
    if us.ndim == 2 and us.shape[0] == m and us.shape[1] >= N:
        return np.ascontiguousarray(np.real(us[:, :N]).T, dtype=np.float64)
    if us.ndim == 3 and us.shape[0] in (1, B) and us.shape[1] == m and us.shape[2] >= N:
        return np.ascontiguousarray(np.real(us[:, :, :N]).transpose(0, 2, 1), dtype=np.float64)
    raise ValueError("us must be a callable of time, (m, >= N) or (B, m, >= N) with m = %d, N = %d, B = %d, got shape %s"
                     % (m, N, B, us.shape))

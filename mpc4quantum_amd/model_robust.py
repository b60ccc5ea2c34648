"""ONE pulse optimised against an ensemble of MODELS in one device call (m4q_model_robust_batch), and the primitive its line search
runs on: S control sequences shared by the ensemble, each rolled through all B members' models in one launch
(m4q_model_rollout_multi_batch).  The model twins of plant_robust.py's two calls: what a dissipative ensemble - the generator plant
has no control gradient of its own - or an ensemble of identified models (dmdc_fit_batch) optimises a robust pulse on.

A model advances by its own step: x+ = A [x ; lift_u(v) (x) x] with v = u_scale[b] * u[t], models [n, n (1 + P)] shared or
[B, n, n (1 + P)] per member (model_rollout_batch).  The objective is plant_robust.py's, F(U) = sum_b w_b J_b(U) with J_b the
figure of model_rollout_grad_batch(reduce=True), and so is the loop: the definition here is plant_robust._loop on
model_rollout_grad_reference(reduce=True) and model_rollout_multi_reference - there is no second loop.

Arrays keep the ensemble axis outermost.  Every shape is checked, and ValueError raised, before the library is touched."""
import numpy as np

from . import _lib
from .grad import _grad_common, _model_member, _models, model_rollout_grad_reference, ordered_weighted_sum
from .library import create_power_list
from .plant_robust import MAX_S, _loop, _robust_params, _shared_sequence
from .rollout import _ptr


def _multi_common(x0, us, models, order, W, target, u_scale, figure, weights):
    us = np.ascontiguousarray(us, dtype=np.float64)
    if us.ndim == 2:
        us = us[None]
    if us.ndim != 3 or min(us.shape) < 1:
        raise ValueError("us must be [S, N, m] (S sequences, each shared by the ensemble) or [N, m], got shape %s" % (us.shape,))
    if us.shape[0] > MAX_S:
        raise ValueError("us holds S = %d sequences, at most %d go into one launch" % (us.shape[0], MAX_S))
    x0, _, _, u_scale, W, target, t_per, q_mode, weights = _grad_common(x0, us[0], u_scale, W, target, figure, weights, True)
    B, n = x0.shape
    models, order, m_per = _models(models, order, B, n, us.shape[2])
    return x0, us, u_scale, models, order, m_per, W, target, t_per, q_mode, weights


# ---------------------------------------------------------------- the definitions
def model_rollout_multi_reference(x0, us, models, order, W, target, u_scale=None, figure="last", weights=None, members=True, mean=True):
    """The definition of model_rollout_multi_batch (same arguments), on the host: {"J": [B, S], "F": [S]}.  A member's objective is
    the figure of grad._model_member's forward pass - q_N, or its N + 1 columns added with t ascending from 0.0 - and F their
    ordered_weighted_sum."""
    x0, us, u_scale, models, order, m_per, W, target, t_per, q_mode, weights = _multi_common(x0, us, models, order, W, target, u_scale,
                                                                                              figure, weights)
    if not (members or mean):
        raise ValueError("members=False with mean=False: nothing to return")
    B, n = x0.shape
    S, N, m = us.shape
    powers = create_power_list(order, m)[1:]
    md, tg = models.reshape(-1, n, models.shape[-1]), target.reshape(-1, n)
    J = np.empty((B, S))
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        for s in range(S):
            q, _, _ = _model_member(x0[b], us[s], sc, md[b if m_per else 0], powers, W, tg[b if t_per else 0], q_mode)
            if q_mode == 2:
                acc = 0.0
                for t in range(N + 1):
                    acc = acc + q[t]
                q = acc
            J[b, s] = q
    out = {}
    if members:
        out["J"] = J
    if mean:
        out["F"] = ordered_weighted_sum(J, weights)
    return out


def model_robust_reference(x0, U0, models, order, W, target, sat, u_scale=None, figure="last", weights=None, iters=10, steps=6, mem=5,
                           step0=0.1, tol=1e-9, gtol=0.0, members=False, evaluate=None, trace=None):
    """The definition of model_robust_batch (same arguments), on the host: plant_robust.py's loop on model_rollout_grad_reference
    with reduce and model_rollout_multi_reference.  evaluate and trace as plant_robust_reference."""
    sat, iters, steps, mem, step0, tol, gtol = _robust_params(sat, iters, steps, mem, step0, tol, gtol)
    U0 = _shared_sequence(U0, "U0")
    if evaluate is None:
        _multi_common(x0, U0, models, order, W, target, u_scale, figure, weights)
        kw = dict(u_scale=u_scale, figure=figure, weights=weights)

        def grad_fn(U):
            out = model_rollout_grad_reference(x0, U, models, order, W, target, reduce=True, **kw)
            return out["q_mean"], out["grad"]

        def roll_fn(us, members=False):
            out = model_rollout_multi_reference(x0, us, models, order, W, target, **kw)
            return (out["F"], out["J"]) if members else out["F"]
    else:
        grad_fn, roll_fn = evaluate
    out = _loop(U0, sat, iters, steps, mem, step0, tol, gtol, grad_fn, roll_fn, trace)
    if members:
        out["J"] = np.asarray(roll_fn(out["U"][None], members=True)[1], dtype=np.float64)[:, 0]
    return out


# ---------------------------------------------------------------- the device
def model_rollout_multi_batch(x0, us, models, order, W, target, u_scale=None, figure="last", weights=None, members=True, mean=True):
    """S control sequences, each shared by the ensemble, rolled through all B members' models in ONE launch: the member's model is
    staged once, not once per sequence.

    x0 [B, n]; us [S, N, m] (1 <= S <= 8) or [N, m]; models, order, u_scale, W, target as model_rollout_grad_batch.  figure: "last"
    -> J = q_N, "sum" -> J = sum_t q_t.  Returns a dict: with members "J" [B, S], the members' objectives - J[:, s] has the bits
    of model_rollout_batch's figure under us[s]; with mean "F" [S] = sum_b w_b J[b, s] in the order of ordered_weighted_sum,
    w = weights [B] or 1 / B."""
    x0, us, u_scale, models, order, m_per, W, target, t_per, q_mode, weights = _multi_common(x0, us, models, order, W, target, u_scale,
                                                                                              figure, weights)
    if not (members or mean):
        raise ValueError("members=False with mean=False: nothing to return")
    B, n = x0.shape
    S, N, m = us.shape
    J = np.empty((B, S), dtype=np.float64) if members else None
    F = np.empty(S, dtype=np.float64) if mean else None
    L = _lib.lib()
    _lib.check(L.m4q_model_rollout_multi_batch(B, n, m, order, N, _ptr(x0), S, _ptr(us), _ptr(u_scale), _ptr(models), m_per, _ptr(W),
                                               _ptr(target), t_per, q_mode, _ptr(weights), _ptr(J), _ptr(F)))
    out = {}
    if members:
        out["J"] = J
    if mean:
        out["F"] = F
    return out


def model_robust_batch(x0, U0, models, order, W, target, sat, u_scale=None, figure="last", weights=None, iters=10, steps=6, mem=5,
                       step0=0.1, tol=1e-9, gtol=0.0, members=False):
    """ONE control sequence optimised against the weighted mean of an ensemble of models, in one device call: plant_robust_batch's
    projected L-BFGS on F(U) = sum_b w_b J_b(U), |U| <= sat, with the members' models in place of their plants.

    x0 [B, n]; U0 [N, m], the first guess shared by the ensemble; models [n, n (1 + P)] or [B|1, n, n (1 + P)], order, u_scale, W,
    target, figure, weights as model_rollout_grad_batch(reduce=True); sat, iters, steps, mem, step0, tol, gtol, members and the
    returned dict as plant_robust_batch."""
    sat, iters, steps, mem, step0, tol, gtol = _robust_params(sat, iters, steps, mem, step0, tol, gtol)
    U0 = _shared_sequence(U0, "U0")
    x0, us, u_scale, models, order, m_per, W, target, t_per, q_mode, weights = _multi_common(x0, U0, models, order, W, target, u_scale,
                                                                                              figure, weights)
    B, n = x0.shape
    N, m = U0.shape
    U, cost = np.empty((N, m)), np.empty(1)
    cost_hist, alpha_hist, pgrad_hist = np.empty(iters + 1), np.empty(iters), np.empty(iters)
    n_iter, status = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    J = np.empty(B) if members else None
    L = _lib.lib()
    _lib.check(L.m4q_model_robust_batch(B, n, m, order, N, _ptr(x0), _ptr(U0), _ptr(u_scale), _ptr(models), m_per, _ptr(W), _ptr(target),
                                        t_per, q_mode, _ptr(weights), sat, iters, steps, mem, step0, tol, gtol, _ptr(U), _ptr(cost),
                                        _ptr(cost_hist), _ptr(alpha_hist), _ptr(pgrad_hist), n_iter.ctypes.data_as(_lib._ip),
                                        status.ctypes.data_as(_lib._ip), _ptr(J)))
    out = {"U": U, "cost": float(cost[0]), "cost_hist": cost_hist, "alpha_hist": alpha_hist, "pgrad_hist": pgrad_hist,
           "n_iter": int(n_iter[0]), "status": int(status[0])}
    if members:
        out["J"] = J
    return out

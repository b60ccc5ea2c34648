"""Plants.  `Experiment` keeps the reference's duck type (mpc4quantum/experiment.py:8-49: lift, proj,
simulate).  `QExperiment` is the state-preparation plant of experiment.py:175-212 with the ODE
  d rho/dt = -i [H0 + sum_k u_k(t) H_k, rho]
solved exactly over each held-control interval by the HIP Pade-13 kernel (m4q_plant_step_batch)
instead of qutip.mesolve.  `mpc()` recognises it and keeps the whole closed loop on the GPU.
`QSynthesis` is the gate-synthesis plant of experiment.py:336-417: its state is the process vector vec_r(U (x) U^*), stepped
exactly by the same kernel family (M4Q_PLANT_PROCESS) instead of qutip.propagator."""
from abc import ABC, abstractmethod

import numpy as np

from . import _lib
from .feedback import plant_feedback_batch
from .noise import require_noise
from .rollout import held_controls, plant_rollout_batch


class Experiment(ABC):
    device_noise = None          # a MeasurementNoise mpc() adds on the device (QExperiment.set_noise, QSynthesis.set_noise)

    def __init__(self):
        self.ts = None
        self.us = None
        self.xs = None

    @abstractmethod
    def f(self, t, x, u):
        """Time derivative of the state."""

    @staticmethod
    def lift(x):
        return x

    @staticmethod
    def proj(z):
        return z

    @abstractmethod
    def simulate(self, x0, ts, us):
        """States at all times in ts, shape (n, len(ts))."""


def _as_array(op):
    return np.asarray(op.full() if hasattr(op, "full") else op, dtype=np.complex128)


def plant_step_batch(x, u, op0, ops, dt, kind=_lib.PLANT_HAMILTONIAN):
    """x [B,n], u [B,m], op0 [B|1,k,k] (or [k,k]), ops [B|1,m,k,k] (or [m,k,k]) -> x_next [B,n].
    k = d for HAMILTONIAN (n = d^2) and PROCESS (n = d^4), n for GENERATOR."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    u = np.ascontiguousarray(u, dtype=np.float64)
    Bn, n = x.shape
    m = u.shape[1]
    op0 = np.ascontiguousarray(op0, dtype=np.complex128)
    ops = np.ascontiguousarray(ops, dtype=np.complex128)
    if int(kind) == _lib.PLANT_PROCESS:
        d = process_dim(n)
        if op0.shape[-2:] != (d, d) or ops.shape[-3:] != (m, d, d) or op0.ndim not in (2, 3) or ops.ndim not in (3, 4):
            raise ValueError("process plant of n = %d = %d^4: op0 must be [B|1, %d, %d] and ops [B|1, %d, %d, %d], got %s and %s"
                             % (n, d, d, d, m, d, d, op0.shape, ops.shape))
    per = 1 if (op0.ndim == 3 and op0.shape[0] > 1) else 0
    if per and (ops.ndim == 3 or ops.shape[0] == 1):
        # per-member op0 with one shared set of control operators: the kernel reads both with the member's stride
        ops = np.ascontiguousarray(np.broadcast_to(ops.reshape((-1,) + ops.shape[-3:])[:1], (Bn,) + ops.shape[-3:]))
    out = np.empty_like(x)
    L = _lib.lib()
    _lib.check(L.m4q_plant_step_batch(Bn, n, m, int(kind), float(dt), _lib.cbuf(x)[1], _lib.rbuf(u)[1], _lib.cbuf(op0)[1],
                                      _lib.cbuf(ops)[1], per, out.ctypes.data_as(_lib._dp)))
    return out


def _simulate_batch(exp, x0s, ts, us, op0, u_scale, W, target, keep, figure):
    """simulate_batch of the three device plants: the plant's own operators() unless per-member op0 [B, k, k] is given."""
    x0s = np.asarray(x0s, dtype=np.complex128)
    if x0s.ndim == 1:
        x0s = x0s[None]
    own0, ops = exp.operators()
    u = held_controls(us, ts, len(exp.H1_list), x0s.shape[0])
    return plant_rollout_batch(x0s, u, own0 if op0 is None else op0, ops, ts, exp.plant_kind, u_scale=u_scale, W=W, target=target,
                               keep=keep, figure=figure)


def _feedback_batch(exp, x0s, ts, law, op0, u_scale, noise, W, target, keep, figure, controls):
    """feedback_batch of the three device plants: simulate_batch's arguments, a FeedbackLaw in the controls' place."""
    x0s = np.asarray(x0s, dtype=np.complex128)
    if x0s.ndim == 1:
        x0s = x0s[None]
    own0, ops = exp.operators()
    return plant_feedback_batch(x0s, law, own0 if op0 is None else op0, ops, ts, exp.plant_kind, u_scale=u_scale, noise=noise, W=W,
                                target=target, keep=keep, figure=figure, controls=controls)


def _gradient_batch(exp, x0s, ts, us, W, target, op0, u_scale, figure, weights, reduce, scale_grad):
    """gradient_batch of the two unitary device plants: simulate_batch's arguments into plant_rollout_grad_batch."""
    from .grad import plant_rollout_grad_batch
    x0s = np.asarray(x0s, dtype=np.complex128)
    if x0s.ndim == 1:
        x0s = x0s[None]
    own0, ops = exp.operators()
    u = held_controls(us, ts, len(exp.H1_list), x0s.shape[0])
    return plant_rollout_grad_batch(x0s, u, own0 if op0 is None else op0, ops, ts, W, target, exp.plant_kind, u_scale=u_scale,
                                    figure=figure, weights=weights, reduce=reduce, scale_grad=scale_grad)


def _calibrate_batch(exp, x0s, ts, us, dirs, W, data, op0, kwargs):
    """calibrate_batch of the two unitary device plants: simulate_batch's arguments into plant_calibrate_batch."""
    from .plant_param import plant_calibrate_batch
    x0s = np.asarray(x0s, dtype=np.complex128)
    if x0s.ndim == 1:
        x0s = x0s[None]
    own0, ops = exp.operators()
    u = held_controls(us, ts, len(exp.H1_list), x0s.shape[0])
    return plant_calibrate_batch(x0s, u, own0 if op0 is None else op0, ops, dirs, ts, W, data, kind=exp.plant_kind, **kwargs)


def _linearize_batch(exp, X, U, ts_or_dt, u_scale, outputs, op0):
    """linearize_batch of the two unitary device plants: the plant's own operators() unless per-member op0 [B, k, k] is given."""
    from .plant_linearize import plant_linearize_batch
    own0, ops = exp.operators()
    return plant_linearize_batch(X, U, own0 if op0 is None else op0, ops, ts_or_dt, exp.plant_kind, u_scale=u_scale, outputs=outputs)


def _quad_program_batch(exp, X, U, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, u_scale, exact, gains, op0):
    """quad_program_batch of the two unitary device plants, on their own linearisation: operators as _linearize_batch."""
    from .plant_linearize import plant_quad_program_batch
    own0, ops = exp.operators()
    return plant_quad_program_batch(X, U, own0 if op0 is None else op0, ops, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du=du, u_prev=u_prev,
                                    x_init=x_init, kind=exp.plant_kind, u_scale=u_scale, exact=exact, gains=gains)


def _sqp_batch(exp, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0):
    """plant_sqp_batch of the two unitary device plants: operators as _linearize_batch."""
    from .plant_sqp import plant_sqp_batch
    own0, ops = exp.operators()
    return plant_sqp_batch(x0, U0, own0 if op0 is None else op0, ops, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=iters, steps=steps,
                           tol=tol, du=du, u_prev=u_prev, kind=exp.plant_kind, u_scale=u_scale, exact=exact, gains=gains)


def _robust_batch(exp, x0, U0, ts_or_dt, W, target, sat, op0, u_scale, figure, weights, iters, steps, mem, step0, tol, gtol, members):
    """plant_robust_batch of the two unitary device plants: operators as _linearize_batch."""
    from .plant_robust import plant_robust_batch
    own0, ops = exp.operators()
    return plant_robust_batch(x0, U0, own0 if op0 is None else op0, ops, ts_or_dt, W, target, sat, kind=exp.plant_kind, u_scale=u_scale,
                              figure=figure, weights=weights, iters=iters, steps=steps, mem=mem, step0=step0, tol=tol, gtol=gtol,
                              members=members)


def _robust_model_batch(exp, x0, U0, dt, order, W, target, sat, op0, u_scale, figure, weights, iters, steps, mem, step0, tol, gtol, members):
    """model_robust_batch on the discretised generators of any plant kind: operators() in generator form (liouvillian(H) for a
    Hamiltonian plant, the generators as they stand otherwise), the per-member op0 [B, k, k] in that same form in place of the
    drift.  Everything is checked before the library is touched - the discretisation included."""
    from .grad import _grad_common
    from .model_robust import model_robust_batch
    from .plant_robust import _robust_params, _shared_sequence
    from .vectorize import discretize_homogeneous, discretize_homogeneous_batch, liouvillian
    if np.ndim(dt) != 0:
        raise ValueError("robust_model_batch takes a scalar dt, got an array of shape %s: a model advances by its own step, so a time "
                         "grid has no meaning here (robust_batch takes one, on the plants that have a gradient)" % (np.shape(dt),))
    dt = float(dt)
    if not (dt > 0 and np.isfinite(dt)):
        raise ValueError("dt must be positive and finite, got %r" % (dt,))
    if isinstance(order, bool) or int(order) != order or not 1 <= int(order) <= 4:
        raise ValueError("order must be an integer in 1..4, got %r" % (order,))
    order = int(order)
    _robust_params(sat, iters, steps, mem, step0, tol, gtol)
    U0 = _shared_sequence(U0, "U0")
    x0c = _grad_common(x0, U0, u_scale, W, target, figure, weights, True)[0]
    B, n = x0c.shape
    own0, ops = exp.operators()
    m = len(ops)
    if U0.shape[1] != m:
        raise ValueError("U0 must be [N, m] = (.., %d) for this plant's %d control operators, got %s" % (m, m, U0.shape))
    k = own0.shape[0]
    generator = exp.plant_kind == _lib.PLANT_GENERATOR
    if (k if generator else k * k) != n:
        raise ValueError("x0 must be [B, n] with n = %d for this plant, got %s" % (k if generator else k * k, x0c.shape))
    if op0 is not None:
        op0 = np.asarray(op0, dtype=np.complex128)
        if op0.shape != (B, k, k):
            raise ValueError("op0 must be [B, k, k] = (%d, %d, %d), got %s" % (B, k, k, op0.shape))
    drift = own0 if op0 is None else op0
    gens = [drift if generator else liouvillian(drift)] + [g if generator else liouvillian(g) for g in ops]
    if order <= 2:
        models = discretize_homogeneous_batch(gens, dt, order)
        models = models if op0 is not None else models[0]
    else:                                                         # (no device discretisation beyond order 2: m4q_discretize_batch)
        models = discretize_homogeneous([np.broadcast_to(g, (B, n, n)) for g in gens] if op0 is not None else gens, dt, order)
    out = model_robust_batch(x0, U0, models, order, W, target, sat, u_scale=u_scale, figure=figure, weights=weights, iters=iters,
                             steps=steps, mem=mem, step0=step0, tol=tol, gtol=gtol, members=members)
    out["models"] = models
    return out


def _ilqr_batch(exp, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0):
    """plant_ilqr_batch of the two unitary device plants: operators as _linearize_batch."""
    from .plant_ilqr import plant_ilqr_batch
    own0, ops = exp.operators()
    return plant_ilqr_batch(x0, U0, own0 if op0 is None else op0, ops, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=iters, steps=steps,
                            tol=tol, du=du, u_prev=u_prev, kind=exp.plant_kind, u_scale=u_scale, exact=exact, gains=gains)


class QExperiment(Experiment):
    """Closed-system plant: H0 and H1_list are d x d Hermitian (ndarray or qutip.Qobj)."""

    def __init__(self, H0, H1_list):
        super().__init__()
        self.H0 = _as_array(H0)
        self.H1_list = [_as_array(h) for h in H1_list]
        self._me_args = {}
        self._sigma = 0

    def set(self, key, value):
        """Keyword argument of the reference's mesolve call (experiment.py:196-200).  The ones that change the ODE or its
        output are honoured: 'c_ops' (collapse operators: the plant becomes the Lindblad generator, still exact per held
        interval, still fused into the closed loop) and 'e_ops' (simulate returns expectation values, experiment.py:210).
        Anything else ('options', 'args', 'progress_bar', ...) only tunes qutip's integrator and is kept but unused."""
        self._me_args[key] = value

    def _c_ops(self):
        return [_as_array(c) for c in (self._me_args.get("c_ops") or [])]

    @property
    def plant_kind(self):
        return _lib.PLANT_GENERATOR if self._c_ops() else _lib.PLANT_HAMILTONIAN

    def operators(self):
        """(op0, ops) for the device plant: the Hamiltonians, or with collapse operators the generators on vec_r(rho)
        L0 = -i[H0, .] + sum_c (C . C^H - 1/2 {C^H C, .}),  L_k = -i[H_k, .]."""
        cs = self._c_ops()
        if not cs:
            return self.H0, np.stack(self.H1_list)
        from .vectorize import liouvillian
        d = self.H0.shape[0]
        eye = np.identity(d)
        L0 = liouvillian(self.H0)
        for c in cs:
            cc = c.conj().T @ c
            L0 = L0 + np.kron(c, c.conj()) - 0.5 * (np.kron(cc, eye) + np.kron(eye, cc.T))
        return L0, np.stack([liouvillian(h) for h in self.H1_list])

    def f(self, t, x, u):
        if self._c_ops():
            L0, Lk = self.operators()
            return (L0 + sum(l * uk for l, uk in zip(Lk, np.reshape(u, -1)))) @ np.reshape(x, -1)
        d = self.H0.shape[0]
        H = self.H0 + sum(h * uk for h, uk in zip(self.H1_list, np.reshape(u, -1)))
        rho = np.reshape(x, (d, d))
        return (-1j * (H @ rho - rho @ H)).reshape(-1)

    def set_sigma(self, sigma):
        self._sigma = sigma

    def set_noise(self, noise):
        """Measurement noise mpc() adds on the device (a MeasurementNoise, or None): unlike set_sigma - np.random on the host, one
        launch per MPC step - the closed loop stays fused and the run is reproducible from the seed.  simulate() itself stays
        noise-free; mpc() refuses an experiment with both this and a non-zero sigma."""
        self.device_noise = require_noise(noise, "QExperiment.set_noise")

    def simulate(self, x0, ts, us):
        """Piecewise-constant control (interp1d kind='previous', mpc.py:258): `us` is a callable of
        time or an (m, len(ts)) array whose column i is held on [ts[i], ts[i+1])."""
        ts = np.asarray(ts, dtype=float)
        m = len(self.H1_list)
        x = np.reshape(np.asarray(x0, dtype=np.complex128), -1)
        (op0, ops), kind = self.operators(), self.plant_kind
        cols = [x]
        for i in range(len(ts) - 1):
            u = np.reshape(us(ts[i]) if callable(us) else np.atleast_2d(us)[:, i], -1)[:m]
            x = plant_step_batch(x[None], np.real(u)[None], op0, ops, ts[i + 1] - ts[i], kind)[0]
            cols.append(x)
        self.ts, self.us = ts, us
        self.xs = np.stack(cols, axis=1)
        e_ops = self._me_args.get("e_ops")
        if e_ops is not None:                                # np.array(res.expect): tr(E rho(t)), one row per operator
            d = self.H0.shape[0]
            rho = self.xs.T.reshape(-1, d, d)
            self.xs = np.array([np.einsum('ij,tji->t', _as_array(e), rho) for e in e_ops])
        if self._sigma:
            noise = np.random.randn(*self.xs.shape) + 1j * np.random.randn(*self.xs.shape)
            return self.xs + noise * self._sigma
        return self.xs

    def simulate_batch(self, x0s, ts, us, op0=None, u_scale=None, W=None, target=None, keep="all", figure="none"):
        """simulate() for an ensemble in one launch (plant_rollout_batch): x0s [B, n]; `us` as simulate() takes it - a callable of
        time or an (m, len(ts)) array, one sequence for all members - or (B, m, len(ts)) per member; op0 [B, k, k]: the members' own
        drift operators in place of this plant's (of operators(): the Lindblad generator when there are collapse operators);
        u_scale [B, m]: the members' drive-amplitude factors.  Returns the dict of plant_rollout_batch: "xs" [B, len(ts), n] (ensemble
        axis first) and / or "q".  Noise-free, and no expectation values: e_ops, set_sigma and set_noise act on simulate() and mpc()."""
        return _simulate_batch(self, x0s, ts, us, op0, u_scale, W, target, keep, figure)

    def feedback_batch(self, x0s, ts, law, op0=None, u_scale=None, noise=None, W=None, target=None, keep="all", figure="none",
                       controls=True):
        """simulate_batch with a stored FeedbackLaw closing the loop (plant_feedback_batch): at every point of ts but the last the
        law reads each member's state and its control is held to the next point.  x0s, ts, op0, u_scale, W, target, keep, figure as
        simulate_batch; noise: a MeasurementNoise added to every stored state but x0s, or None (set_noise and set_sigma act on mpc()
        and simulate()).  Returns plant_feedback_batch's dict: "xs", "q", "us" [B, len(ts) - 1, m], "clipped", "status"."""
        return _feedback_batch(self, x0s, ts, law, op0, u_scale, noise, W, target, keep, figure, controls)

    def gradient_batch(self, x0s, ts, us, W, target, op0=None, u_scale=None, figure="last", weights=None, reduce=False,
                       scale_grad=False):
        """The figure of simulate_batch's rollout and its gradient with respect to the held controls, for an ensemble in one launch
        (plant_rollout_grad_batch): x0s, ts, us, op0, u_scale as simulate_batch; figure "last" (J = q_N) or "sum" (J = sum_t q_t).
        Returns its dict: "q", "grad" [B, N, m] with N = len(ts) - 1 (ensemble axis first, then time, then control), "grad_scale",
        "q_mean".  With collapse operators the plant is a generator plant, which the library refuses: take the gradient of the
        discretised model (model_rollout_grad_batch)."""
        return _gradient_batch(self, x0s, ts, us, W, target, op0, u_scale, figure, weights, reduce, scale_grad)

    def calibrate_batch(self, x0s, ts, us, dirs, W, data, op0=None, **kwargs):
        """Fits this plant's parameters member by member to measured trajectories (plant_calibrate_batch): x0s, ts, us, op0 as
        simulate_batch - op0 the nominal drift, this plant's own unless given -, dirs [p, d, d] or [B|1, p, d, d] the Hermitian
        directions of the drift, data [B|1, len(ts), n] what was measured, the keywords plant_calibrate_batch's (theta0, bounds,
        fit_scale, u_scale, col_w, iters, mem, steps, tol, gtol, step0).  Returns its dict.  With collapse operators the plant is a
        generator plant, which is refused as it is there."""
        if self.plant_kind == _lib.PLANT_GENERATOR:
            raise ValueError("QExperiment.calibrate_batch: with collapse operators the plant is a generator plant, which has no "
                             "parameter gradient on the device - fit the parameters through its discretised model")
        return _calibrate_batch(self, x0s, ts, us, dirs, W, data, op0, kwargs)

    def linearize_batch(self, X, U, ts_or_dt, u_scale=None, outputs=("A", "B", "Delta"), op0=None):
        """The exact Jacobians of this plant's held-control step along trajectories, for an ensemble in one launch
        (plant_linearize_batch): X [B, T, n] the points (ensemble axis first, then time), U [T, m] or [B, T, m] the controls held
        from each, ts_or_dt a scalar dt or a time grid of T + 1 points, u_scale and op0 as simulate_batch.  Returns (A, B, Delta),
        None for an output not asked for.  With collapse operators the plant is a generator plant, which is refused: linearise the
        discretised model (WrapModel.linearize_batch)."""
        return _linearize_batch(self, X, U, ts_or_dt, u_scale, outputs, op0)

    def quad_program_batch(self, X, U, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du=None, u_prev=None, x_init=None, u_scale=None,
                           exact=False, gains=True, op0=None):
        """The QP of quad_program_batch on this plant's own Jacobians along X, U, for an ensemble in one device call
        (plant_quad_program_batch): X, U, ts_or_dt, u_scale, op0 as linearize_batch, the rest as plant_quad_program_batch.  Returns
        (X_opt, U_opt, cost, gains).  With collapse operators the plant is a generator plant, which is refused as it is there."""
        return _quad_program_batch(self, X, U, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, u_scale, exact, gains, op0)

    def sqp_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None, u_scale=None,
                  exact=False, gains=False, op0=None):
        """Controls optimised on this plant itself by a Gauss-Newton SQP, for an ensemble in one device call (plant_sqp_batch):
        x0 [B, n], U0 [T, m] or [B, T, m], ts_or_dt, u_scale, op0 as linearize_batch, the rest as plant_sqp_batch.  Returns its
        dict.  With collapse operators the plant is a generator plant, which is refused as it is there."""
        return _sqp_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0)

    def ilqr_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None, u_scale=None,
                   exact=False, gains=False, op0=None):
        """sqp_batch with the line search run in closed loop - each QP's gains applied on this plant itself (plant_ilqr_batch):
        the same arguments, the same dict, the same refusal of a generator plant."""
        return _ilqr_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0)

    def robust_batch(self, x0, U0, ts_or_dt, W, target, sat, op0=None, u_scale=None, figure="last", weights=None, iters=10, steps=6,
                     mem=5, step0=0.1, tol=1e-9, gtol=0.0, members=False):
        """ONE control sequence U [N, m] optimised against the weighted mean of an ensemble of this plant - per-member op0 [B, k, k]
        and u_scale [B, m] as simulate_batch - by a projected L-BFGS in one device call (plant_robust_batch): x0 [B, n], U0 [N, m],
        ts_or_dt as linearize_batch, the rest and the returned dict as plant_robust_batch.  With collapse operators the plant is a
        generator plant, which is refused."""
        return _robust_batch(self, x0, U0, ts_or_dt, W, target, sat, op0, u_scale, figure, weights, iters, steps, mem, step0, tol, gtol,
                             members)

    def robust_model_batch(self, x0, U0, dt, order, W, target, sat, op0=None, u_scale=None, figure="last", weights=None, iters=10,
                           steps=6, mem=5, step0=0.1, tol=1e-9, gtol=0.0, members=False):
        """robust_batch on the members' discretised MODELS (model_robust_batch): the optimiser every plant kind has, collapse
        operators and LExperiment included.  The generators are those of operators() - for a Hamiltonian plant liouvillian(H),
        with collapse operators or on an LExperiment the generators as they stand - with the per-member op0 [B, k, k] in the same
        form in place of the drift; they are discretised to `order` over the scalar step dt (orders 1-2 on the device, 3-4 on the
        host) into [B, n, n (1 + P)] models, and one U [N, m] is optimised against their weighted mean.  The rest and the returned
        dict as model_robust_batch; the dict gains "models".  A time grid is refused: a model advances by its own step."""
        return _robust_model_batch(self, x0, U0, dt, order, W, target, sat, op0, u_scale, figure, weights, iters, steps, mem, step0, tol,
                                   gtol, members)


class LExperiment(QExperiment):
    """Open-system plant: x' = (L0 + sum_k u_k L_k) x with n x n generators on vec_r(rho)."""

    plant_kind = _lib.PLANT_GENERATOR

    def operators(self):
        return self.H0, np.stack(self.H1_list)

    def gradient_batch(self, *args, **kwargs):
        """Refused: the generator plant has no gradient kernel."""
        raise ValueError("LExperiment.gradient_batch: the generator plant has no control gradient on the device - discretise the "
                         "generators (discretize_homogeneous) and take the gradient of the model with model_rollout_grad_batch")

    def calibrate_batch(self, *args, **kwargs):
        """Refused: the generator plant has no parameter-gradient kernel."""
        raise ValueError("LExperiment.calibrate_batch: the generator plant has no parameter gradient on the device - fit the "
                         "parameters through the discretised model (discretize_homogeneous, model_rollout_grad_batch)")

    def linearize_batch(self, *args, **kwargs):
        """Refused: the generator plant has no linearisation kernel."""
        raise ValueError("LExperiment.linearize_batch: the generator plant has no linearisation of its own on the device - discretise "
                         "the generators (discretize_homogeneous) and linearise the model with WrapModel.linearize_batch")

    def quad_program_batch(self, *args, **kwargs):
        """Refused: the generator plant has no linearisation kernel."""
        raise ValueError("LExperiment.quad_program_batch: the generator plant has no linearisation of its own on the device - "
                         "discretise the generators (discretize_homogeneous), linearise the model with WrapModel.linearize_batch and "
                         "solve with quad_program_batch")

    def robust_batch(self, *args, **kwargs):
        """Refused: the generator plant has no gradient kernel."""
        raise ValueError("LExperiment.robust_batch: the generator plant has no control gradient on the device - discretise the "
                         "generators (discretize_homogeneous) and optimise on the model's gradient (model_rollout_grad_batch)")

    def f(self, t, x, u):
        L = self.H0 + sum(h * uk for h, uk in zip(self.H1_list, np.reshape(u, -1)))
        return L @ np.reshape(x, -1)

    def simulate(self, x0, ts, us):
        ts = np.asarray(ts, dtype=float)
        m = len(self.H1_list)
        x = np.reshape(np.asarray(x0, dtype=np.complex128), -1)
        cols = [x]
        for i in range(len(ts) - 1):
            u = np.reshape(us(ts[i]) if callable(us) else np.atleast_2d(us)[:, i], -1)[:m]
            x = plant_step_batch(x[None], np.real(u)[None], self.H0, np.stack(self.H1_list), ts[i + 1] - ts[i],
                                 _lib.PLANT_GENERATOR)[0]
            cols.append(x)
        self.ts, self.us = ts, us
        self.xs = np.stack(cols, axis=1)
        return self.xs


def process_dim(n):
    """d with d^4 = n: the unitary dimension of a process vector of length n (ValueError otherwise)."""
    n = int(n)
    d = int(round(n ** 0.25))
    if d < 1 or d ** 4 != n:
        raise ValueError("a process vector has d^4 entries; %d is not a fourth power" % n)
    return d


class QSynthesis(Experiment):
    """Gate-synthesis plant (experiment.py:336-417): H0 and H1_list are d x d Hermitian (ndarray or qutip.Qobj).

    The loop state is the process vector P = vec_r(U (x) U^*) (n = d^4), and mpc() does NOT lift it: the lift in the loop is the
    identity (difference 4 - the reference's QSynthesis cannot drive its own mpc.py, whose lift of a process vector
    has d^8 entries).  `lift(U)` / `proj(P)` keep the reference's meaning (U <-> U (x) U^*, proj up to a global phase) as helpers.
    simulate() steps the process vector itself, exactly over each held-control interval (M4Q_PLANT_PROCESS):
    P+ = vec_r((V (x) V^*) M), V = expm(-i dt (H0 + sum_k u_k H_k)) - qutip.propagator's U(t) applied to the state, without it."""

    plant_kind = _lib.PLANT_PROCESS

    def __init__(self, H0, H1_list):
        super().__init__()
        self.H0 = _as_array(H0)
        self.H1_list = [_as_array(h) for h in H1_list]
        self._prop_args = {}

    def set(self, key, value):
        """Keyword argument of the reference's propagator call (experiment.py:354-358): kept and ignored, as QExperiment keeps
        the integrator's options - except 'c_ops': open-system process maps are not a unitary's process vector."""
        if key == "c_ops" and value is not None and len(value):
            raise ValueError("QSynthesis: collapse operators (c_ops) are not supported - the process plant propagates a unitary's "
                             "process vector U (x) U^*; open-system process maps are out of scope")
        self._prop_args[key] = value

    def set_noise(self, noise):
        """Measurement noise mpc() adds on the device (a MeasurementNoise of kind "iid", or None): see QExperiment.set_noise."""
        self.device_noise = require_noise(noise, "QSynthesis.set_noise")

    def operators(self):
        """(op0, ops) for the device plant: the d x d Hamiltonians."""
        return self.H0, np.stack(self.H1_list)

    def f(self, t, x, u):
        """dP/dt = (L (x) I) P with L = -i (H (x) I - I (x) H^*), P = vec_r(M) (M' = L M)."""
        d = self.H0.shape[0]
        H = self.H0 + sum(h * uk for h, uk in zip(self.H1_list, np.reshape(u, -1)))
        eye = np.identity(d)
        L = -1j * (np.kron(H, eye) - np.kron(eye, H.conj()))
        return (L @ np.reshape(x, (d * d, d * d))).reshape(-1)

    @staticmethod
    def lift(U):
        """experiment.py:364-375: flat d x d unitary (d^2,) -> flat process vector vec_r(U (x) U^*) (d^4,)."""
        U = np.asarray(U)
        n = isqrt(U.shape[0])
        U = U.reshape(n, n)
        return np.kron(U, U.conj()).flatten()

    @staticmethod
    def proj(P):
        """experiment.py:377-394: flat process vector (d^4,) -> a flat unitary (d^2,) equal to U up to a global phase: the first
        non-zero d x d block U_ab U^* of P, conjugated and divided by the square root of its own entry (a, b) = |U_ab|^2."""
        P = np.asarray(P)
        n = isqrt(isqrt(P.shape[0]))
        blocks = split_blocks(P.reshape(n ** 2, n ** 2), n, n)
        U = np.zeros((n, n))
        for i, val in enumerate([np.any(b) for b in blocks]):
            if val:
                U = blocks[i].conj() / np.emath.sqrt(blocks[i].flatten()[i])
                break
        return U.flatten()

    def simulate(self, x0, ts, us):
        """Process vectors in, process vectors out (experiment.py:396-417), shape (n, len(ts)); column 0 is x0.  Piecewise-constant
        control as QExperiment.simulate: `us` is a callable of time or an (m, len(ts)) array whose column i is held on
        [ts[i], ts[i+1])."""
        ts = np.asarray(ts, dtype=float)
        m = len(self.H1_list)
        x = np.reshape(np.asarray(x0, dtype=np.complex128), -1)
        op0, ops = self.operators()
        cols = [x]
        for i in range(len(ts) - 1):
            u = np.reshape(us(ts[i]) if callable(us) else np.atleast_2d(us)[:, i], -1)[:m]
            x = plant_step_batch(x[None], np.real(u)[None], op0, ops, ts[i + 1] - ts[i], _lib.PLANT_PROCESS)[0]
            cols.append(x)
        self.ts, self.us = ts, us
        self.xs = np.stack(cols, axis=1)
        return self.xs

    def simulate_batch(self, x0s, ts, us, op0=None, u_scale=None, W=None, target=None, keep="all", figure="none"):
        """simulate() for an ensemble in one launch (plant_rollout_batch): x0s [B, n]; `us` as simulate() takes it - a callable of
        time or an (m, len(ts)) array, one sequence for all members - or (B, m, len(ts)) per member; op0 [B, k, k]: the members' own
        drift operators in place of this plant's (d x d Hamiltonians);
        u_scale [B, m]: the members' drive-amplitude factors.  Returns the dict of plant_rollout_batch: "xs" [B, len(ts), n] (ensemble
        axis first) and / or "q".  Noise-free, and no expectation values: e_ops, set_sigma and set_noise act on simulate() and mpc()."""
        return _simulate_batch(self, x0s, ts, us, op0, u_scale, W, target, keep, figure)

    def feedback_batch(self, x0s, ts, law, op0=None, u_scale=None, noise=None, W=None, target=None, keep="all", figure="none",
                       controls=True):
        """simulate_batch with a stored FeedbackLaw closing the loop (plant_feedback_batch): at every point of ts but the last the
        law reads each member's state and its control is held to the next point.  x0s, ts, op0, u_scale, W, target, keep, figure as
        simulate_batch; noise: a MeasurementNoise added to every stored state but x0s, or None (set_noise and set_sigma act on mpc()
        and simulate()).  Returns plant_feedback_batch's dict: "xs", "q", "us" [B, len(ts) - 1, m], "clipped", "status"."""
        return _feedback_batch(self, x0s, ts, law, op0, u_scale, noise, W, target, keep, figure, controls)

    def gradient_batch(self, x0s, ts, us, W, target, op0=None, u_scale=None, figure="last", weights=None, reduce=False,
                       scale_grad=False):
        """The figure of simulate_batch's rollout and its gradient with respect to the held controls, for an ensemble in one launch
        (plant_rollout_grad_batch on the process plant): arguments and the returned dict as QExperiment.gradient_batch."""
        return _gradient_batch(self, x0s, ts, us, W, target, op0, u_scale, figure, weights, reduce, scale_grad)

    def calibrate_batch(self, x0s, ts, us, dirs, W, data, op0=None, **kwargs):
        """Fits the process plant's parameters member by member to measured process vectors (plant_calibrate_batch): arguments and
        the returned dict as QExperiment.calibrate_batch, data [B|1, len(ts), d^4]."""
        return _calibrate_batch(self, x0s, ts, us, dirs, W, data, op0, kwargs)

    def linearize_batch(self, X, U, ts_or_dt, u_scale=None, outputs=("A", "B", "Delta"), op0=None):
        """The exact Jacobians of the process plant's held-control step along trajectories, for an ensemble in one launch
        (plant_linearize_batch): arguments and the returned tuple as QExperiment.linearize_batch, X [B, T, d^4] process vectors."""
        return _linearize_batch(self, X, U, ts_or_dt, u_scale, outputs, op0)

    def quad_program_batch(self, X, U, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du=None, u_prev=None, x_init=None, u_scale=None,
                           exact=False, gains=True, op0=None):
        """The QP of quad_program_batch on the process plant's own Jacobians along X, U, for an ensemble in one device call
        (plant_quad_program_batch): arguments and the returned tuple as QExperiment.quad_program_batch, X [B, T, d^4]."""
        return _quad_program_batch(self, X, U, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, du, u_prev, x_init, u_scale, exact, gains, op0)

    def sqp_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None, u_scale=None,
                  exact=False, gains=False, op0=None):
        """Controls optimised on the process plant itself by a Gauss-Newton SQP, for an ensemble in one device call
        (plant_sqp_batch): arguments and the returned dict as QExperiment.sqp_batch, x0 [B, d^4] process vectors."""
        return _sqp_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0)

    def ilqr_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters=10, steps=6, tol=1e-9, du=None, u_prev=None, u_scale=None,
                   exact=False, gains=False, op0=None):
        """sqp_batch with the line search run in closed loop on the process plant (plant_ilqr_batch): arguments and the returned
        dict as QExperiment.ilqr_batch, x0 [B, d^4] process vectors."""
        return _ilqr_batch(self, x0, U0, ts_or_dt, X_bm, U_bm, Q_ls, R_ls, sat, iters, steps, tol, du, u_prev, u_scale, exact, gains, op0)

    def robust_batch(self, x0, U0, ts_or_dt, W, target, sat, op0=None, u_scale=None, figure="last", weights=None, iters=10, steps=6,
                     mem=5, step0=0.1, tol=1e-9, gtol=0.0, members=False):
        """ONE control sequence optimised against the weighted mean of an ensemble of process plants in one device call
        (plant_robust_batch): arguments and the returned dict as QExperiment.robust_batch, x0 [B, d^4] process vectors."""
        return _robust_batch(self, x0, U0, ts_or_dt, W, target, sat, op0, u_scale, figure, weights, iters, steps, mem, step0, tol, gtol,
                             members)


def split_blocks(bmatrix, nrows, ncols):
    """experiment.py:309-315: the (nrows x ncols) tiles of a block matrix, row-major over the tiles."""
    bmatrix = np.asarray(bmatrix)
    tiles_down, tiles_across = bmatrix.shape[0] // nrows, bmatrix.shape[1] // ncols
    return np.stack([bmatrix[a * nrows:(a + 1) * nrows, b * ncols:(b + 1) * ncols]
                     for a in range(tiles_down) for b in range(tiles_across)])


def isqrt(n):
    """Integer square root (experiment.py:311-327)."""
    import math
    if n < 0:
        raise ValueError("Square root not defined for negative numbers.")
    return math.isqrt(int(n))


class QExperiment32(QExperiment):
    """Three-level plant seen through its qubit block (experiment.py:215-235): the model lives on the 2x2 block."""

    observe_kind = _lib.OBSERVE_QUBIT_BLOCK      # what lift is on the device (observe.py): mpc() keeps this class's loop there

    @staticmethod
    def lift(rho33_vec):
        block = np.reshape(np.asarray(rho33_vec, dtype=np.complex128), (3, 3))[:2, :2]
        # Qobj.unit(): divide by the trace norm (sum of singular values)
        return (block / np.linalg.svd(block, compute_uv=False).sum()).flatten()

    @staticmethod
    def proj(rho22_vec):
        return np.asarray(rho22_vec).flatten()          # as the reference returns it (experiment.py:231-235)


class QCoupledExperiment(QExperiment):
    """Two identical subsystems: the model sees the two reduced states [vec(rho_A), vec(rho_B)] (partial traces),
    the plant the joint state (experiment.py:238-306)."""

    observe_kind = _lib.OBSERVE_PARTIAL_TRACE    # what lift is on the device (observe.py): mpc() keeps this class's loop there

    @staticmethod
    def lift(rhoAB_vec):
        v = np.asarray(rhoAB_vec, dtype=np.complex128).reshape(-1)
        dA = isqrt(isqrt(v.size))
        r = v.reshape(dA, dA, dA, dA)                    # r[a, b, a', b'] = <a b| rho |a' b'>
        return np.hstack([np.einsum('abcb->ac', r).flatten(), np.einsum('abad->bd', r).flatten()])

    @staticmethod
    def proj(rhoA_rhoB_vec):
        v = np.asarray(rhoA_rhoB_vec).reshape(-1)
        dA = isqrt(v.size // 2)
        return np.kron(v[:dA * dA].reshape(dA, dA), v[dA * dA:].reshape(dA, dA)).flatten()

"""Receding-horizon driver with the reference's interface (mpc4quantum/mpc.py): StepClock, mpc(),
shift_guess, iqp_line_search, val_to_str, plus the batched mpc_batch().

The loop body of the reference (mpc.py:161-292: linearise along the guess, solve the horizon QP,
line-search, apply U_opt[:,0], propagate the plant, shift) runs inside the persistent HIP kernel
`mpc_kernel` (csrc/m4q_kernels.hip) for every ensemble member at once.  Quirks kept on purpose:
u_prev from U_ref at steps 0 and 1 (:185), applied control U_opt[:,0] (:250), the one-step lag of
the target window (:276-277), exit codes and the dropped last entry (:294-304)."""
import numpy as np

from . import _lib
from .exit_condition import QuadraticExit, require_device_exit
from .experiment import Experiment, QCoupledExperiment, QExperiment, QExperiment32, QSynthesis
from .library import krtimes
from .linearize import WrapModel
from .noise import check_batch_noise, require_noise
from .observe import check_observed_plant, observe_batch, observe_dims
from .session import EnsembleSession


class StepClock:
    """mpc.py:14-35."""

    def __init__(self, dt, horizon, n_steps):
        self.dt = float(dt)
        self.horizon = horizon
        self.n_steps = n_steps
        self.measure_freq = 1
        self.ts = np.linspace(0, self.dt * self.n_steps, self.n_steps, endpoint=False)
        self.ts_sim = self.ts

    def set_endsim(self, index):
        self.ts_sim = self.ts[:index]

    def ts_step(self, a_step):
        return np.linspace(self.dt * (a_step + 1 - self.measure_freq), self.dt * (a_step + 1), self.measure_freq + 1)

    def ts_horizon(self, a_step):
        return np.linspace(self.dt * a_step, self.dt * (a_step + self.horizon), self.horizon, endpoint=False)

    def to_string(self):
        parts = ['mf', val_to_str(self.measure_freq), 'dt', val_to_str(self.dt), 'h', val_to_str(self.horizon), 'n',
                 val_to_str(self.n_steps)]
        return '_'.join(parts)


def val_to_str(val):
    """mpc.py:64-68: 1.0E-02 -> 1d0em02."""
    return f'{val:.1E}'.replace('E', 'e').replace('.', 'd').replace('-', 'm').replace('+', '')


def shift_guess(data):
    """mpc.py:71-73."""
    data = np.asarray(data)
    return np.hstack([data[:, 1:], data[:, -1:]])


def isinf_warning():
    """mpc.py:76-79: what the reference prints on exit code 3."""
    import warnings
    warnings.warn("Solution was infinite (failed to converge). Inspect the model for accuracy, check if control constraints "
                  "can regularize the problem, or run with verbose=True for more information.")


def solver_warning():
    """Exit code 2 (mpc.py:183-197: a solver warning ends the run).  Without OSQP the one solver that can give up is the exact
    box-QP iteration (exact_qp=True) stopping at its iteration cap."""
    import warnings
    warnings.warn("The exact box-QP solve stopped at its iteration cap before reaching the KKT point (exit code 2); "
                  "the horizon QP is too ill-conditioned for fp64 - shorten the horizon or use the clipped solve.")


def complex_to_real(z):
    """mpc.py:87-89: complex vector of length n -> [Re; Im] of length 2n."""
    return np.concatenate((np.real(z), np.imag(z)))


def real_to_complex(z):
    """mpc.py:82-84: the inverse, [Re; Im] -> complex."""
    z = np.asarray(z)
    half = len(z) // 2
    return z[:half] + 1j * z[half:]


def real_to_complex_op(P):
    """mpc.py:96-98: inverse of complex_to_real_op, read off the left block column."""
    P = np.asarray(P)
    r, c = P.shape[0] // 2, P.shape[1] // 2
    return P[:r, :c] + 1j * P[r:, :c]


def complex_to_real_op(P):
    P = np.asarray(P)
    return np.block([[P.real, -P.imag], [P.imag, P.real]])


def iqp_line_search(Q_ls, R_ls, X_htarg, U_htarg, X_guess, U_guess, X_opt, U_opt):
    """Host form of the line search the kernel performs (mpc.py:101-125), same return arity:
    (alpha, new_step, new_fval, new_slope).  Z is stacked and the cost blocks are laid out exactly as
    the reference does (see csrc/m4q_mpc.h line_search)."""
    def pack(X, U):
        xf, uf = np.asarray(X, dtype=complex).flatten(), np.asarray(U, dtype=complex).flatten()
        return np.concatenate((complex_to_real(xf), complex_to_real(uf)))
    Zt, Zg, Zo = pack(X_htarg, U_htarg), pack(X_guess, U_guess), pack(X_opt, U_opt)
    blocks = [complex_to_real_op(q) for q in Q_ls] + [complex_to_real_op(r) for r in R_ls]

    def apply(v):
        out = np.empty_like(v)
        pos = 0
        for b in blocks:
            k = b.shape[0]
            out[pos:pos + k] = 0.5 * (b + b.T) @ v[pos:pos + k]
            pos += k
        return out
    DZ = Zo - Zg
    alpha = -apply(Zg - Zt).dot(DZ) / (DZ @ apply(DZ))
    Zn = Zg + alpha * DZ
    new_fval = 0.5 * (Zn - Zt) @ apply(Zn - Zt)
    return alpha, np.linalg.norm(alpha * DZ), new_fval, apply(Zn - Zt)


def _native_plant(experiment):
    """True if the closed loop can stay on the GPU: one of this package's plants with identity lift/proj."""
    return (isinstance(experiment, QExperiment) and type(experiment).lift is Experiment.lift
            and type(experiment).proj is Experiment.proj and not getattr(experiment, "_sigma", 0)
            and getattr(experiment, "_me_args", {}).get("e_ops") is None)


def _identity(x):
    return x


def _loop_maps(experiment):
    """(lift, proj) the loop applies to the plant's states.  A QSynthesis experiment's loop state IS its process vector: the lift
    in the loop is the identity (difference 4), its lift / proj are helpers between U and U (x) U^*."""
    if isinstance(experiment, QSynthesis):
        return _identity, _identity
    return experiment.lift, experiment.proj


def _trim(xs, us, code, done):
    """mpc.py:294-304: normal exit keeps done+1 states and done controls; an early exit drops the attempted entry."""
    if code == 0:
        return [xs[:, :done + 1], us[:, :done]]
    return [xs[:, :done + 1], us[:, :done] if done > 0 else None]


def _runs_fused(experiment, exit_condition, streaming):
    """mpc() keeps the whole loop in one launch when the plant runs on the device and the exit condition, if any, is one the kernel
    evaluates (a QuadraticExit); a plain callable, a host plant or streaming updates take one launch per MPC step."""
    return ((_native_plant(experiment) or isinstance(experiment, QSynthesis)) and not streaming
            and (exit_condition is None or isinstance(exit_condition, QuadraticExit)))


def _runs_observed(experiment, exit_condition, streaming, measure_freq=1):
    """mpc() keeps the closed loop of an observed plant (observe.py) on the device - one MPC launch and one plant-and-observe launch
    per step, no host round trip - when the experiment's class is exactly QCoupledExperiment or QExperiment32 (a subclass may bring
    its own lift) on the dimensions the kernels are built for, without collapse operators, e_ops, sigma or device noise, with no exit
    condition, no streaming updates and measure_freq 1.  Anything else keeps the host path."""
    if type(experiment) not in (QCoupledExperiment, QExperiment32):
        return False
    d = observe_dims(type(experiment).observe_kind)[2]
    return (np.shape(experiment.H0) == (d, d) and not experiment._c_ops() and experiment._me_args.get("e_ops") is None
            and not experiment._sigma and experiment.device_noise is None and exit_condition is None and not streaming
            and int(measure_freq) == 1)


def mpc(x0, dim_u, order, X_targ, U_targ, clock, experiment, model, Q, R, Qf, sat=None, du=None, max_iter=100,
        exit_condition=None, streaming=False, warm_start=True, progress_bar=True, verbose=False, exact_qp=False,
        qp_flags=None):
    """Drop-in for mpc4quantum.mpc.mpc (mpc.py:128-304): returns ([xs, us], model, exit_code).
    exact_qp (extension): solve each QP to the box-constrained optimum, as the reference's OSQP call does, instead of
    clipping the Riccati rollout (identical whenever no bound is active).
    qp_flags (extension): M4Q_QP_* bits; _lib.QP_REF_LQR runs the loop around the arithmetic of the reference's lqr.py as
    written, which is what tests/golden/mpc_loop.npz (the reference's own mpc.py around its own lqr.py) pins.
    A QSynthesis experiment (gate synthesis) runs on its process vector with the identity as the loop's lift: x0, the states
    returned and the states exit_condition sees are process vectors vec_r(U (x) U^*).
    exit_condition: any callable exit_condition(x_next, x, u) runs the loop on the host, one launch per MPC step; a QuadraticExit
    with a native plant or QSynthesis (and no streaming) keeps the loop fused: the kernel evaluates it after every step.
    Measurement noise: experiment.set_noise(MeasurementNoise(...)) keeps the loop fused - the kernel draws the noise of member
    `member_base` - and a loop that runs step by step for another reason adds the same draws here, after simulate: the same run
    either way.  set_sigma alone is the reference's np.random noise on the host path, as before; both on one experiment raise.
    A QCoupledExperiment or QExperiment32 with default settings (_runs_observed) keeps its loop on the device as an observed plant:
    the same states and controls as the host path returns, to the rounding of the lift and of the loop's conditioning."""
    noise = require_noise(getattr(experiment, "device_noise", None), "mpc (experiment.device_noise)")
    if noise is not None and getattr(experiment, "_sigma", 0):
        raise ValueError("the experiment has both device noise (set_noise) and a non-zero sigma (set_sigma): choose one")
    mf = int(clock.measure_freq)
    x0 = np.asarray(x0, dtype=np.complex128).reshape(-1)
    lift, proj = _loop_maps(experiment)
    observed = _runs_observed(experiment, exit_condition, streaming, mf)
    if observed and x0.shape[0] != observe_dims(experiment.observe_kind)[0]:
        raise ValueError("mpc: x0 has %d entries, the plant state of a %s has %d"
                         % (x0.shape[0], type(experiment).__name__, observe_dims(experiment.observe_kind)[0]))
    # (observed plant: the state the first QP sees is the device's own observation of x0, the one it stores as xs[:, 0])
    lift_x0 = observe_batch(experiment.observe_kind, x0[None])[0] if observed \
        else np.asarray(lift(x0), dtype=np.complex128).reshape(-1)
    A_x, A_u = model.get_discrete()
    wrapped = WrapModel(A_x, A_u, dim_u, order)          # validates the library size like mpc.py:156
    n = wrapped.dim_x
    T, ns = clock.horizon, clock.n_steps
    X_targ = np.atleast_2d(np.asarray(X_targ))
    U_targ = np.atleast_2d(np.asarray(U_targ))
    cols = min(X_targ.shape[1], ns + T + 1)
    fused = _runs_fused(experiment, exit_condition, streaming)
    kind = experiment.plant_kind if fused else _lib.PLANT_NONE
    if noise is not None:                        # (stepwise: added to what simulate returns, in the plant's own space)
        if fused:
            check_batch_noise(noise, 1, n, kind, "mpc")
        else:
            noise.check(1, x0.shape[0])
    # stepwise with "iid" noise: the states handed back (put_state) are not Hermitian, so the QPs run the complex path, as the fused
    # session does of its own accord (m4q_session_set_noise)
    sess = EnsembleSession(1, n, dim_u, order, T, ns, clock.dt, sat, du, max_iter, warm_start, qp_flags=qp_flags,
                           plant_kind=kind, target_cols=cols, measure_freq=mf, exact_qp=exact_qp,
                           force_complex=noise is not None and noise.kind == "iid" and not fused)
    try:
        op0, ops = experiment.operators() if fused else (None, None)
        sess.load_problem(np.hstack([A_x, A_u])[None], lift_x0[None], X_targ, U_targ, Q, R, Qf, op0, ops)
        if fused:
            if exit_condition is not None:
                sess.set_exit_condition(exit_condition)
            if noise is not None:
                sess.set_noise(noise)
            sess.run(0, ns)
            res = sess.results()
            code, done = int(res["exit_codes"][0]), int(res["steps_done"][0])
            if code == 3:
                isinf_warning()                                                                # mpc.py:200-203
            if code == 2:
                solver_warning()                                                               # mpc.py:193-196
            clock.set_endsim(done)
            return _trim(res["xs"][0].T, res["us"][0].T, code, done), model, code
        if observed:
            sess.set_observed_plant(experiment.observe_kind, experiment.H0, np.stack(experiment.H1_list), x0[None])
            sess.run_observed(0, ns)
            sess.sync()
            res = sess.results()
            zs = sess.plant_states()
            code, done = int(res["exit_codes"][0]), int(res["steps_done"][0])
            if code == 3:
                isinf_warning()
            if code == 2:
                solver_warning()
            clock.set_endsim(done)
            return _trim(zs[0].T, res["us"][0].T, code, done), model, code      # (the plant states, as the host path returns them)
        # host plant: one launch per MPC step, the plant (and lift/proj) evaluated by the caller's object
        xs = [x0]
        us = []
        code = 0
        step = 0
        it = range(ns)
        if progress_bar:
            try:
                from tqdm.auto import tqdm
                it = tqdm(it)
            except ImportError:
                pass
        for step in it:
            sess.run(step, step + 1)
            sess.sync()
            dev_code = int(sess.download(_lib.F_CODES, (1,))[0])
            if dev_code:
                code = dev_code
                if code == 3:
                    isinf_warning()
                if code == 2:
                    solver_warning()
                break
            u = sess.download(_lib.F_US, (1, ns, dim_u))[0, step]
            us.append(u)
            if (step + 1) % mf == 0:
                # measure: plant from the last measured state; controls stacked newest first as mpc.py:257 does
                ts_step = clock.ts_step(step)
                us_step = np.vstack([us[step - jq] for jq in range(mf)] + [us[step]]).T
                result = experiment.simulate(xs[step + 1 - mf], ts_step, _HeldControl(ts_step, us_step))   # mpc.py:256-260
                x_meas = np.asarray(result)[:, -1]
                if noise is not None:                    # the draws the fused loop makes for this member and column of xs
                    x_meas = x_meas + noise.sample([0], step + 1, x_meas.shape[0])[0]
                xs.append(x_meas)
            else:
                lx = np.asarray(lift(xs[step])).reshape(-1, 1)                                 # mpc.py:261-267
                lu = wrapped.lift_u(u.reshape(-1, 1))
                xs.append(np.asarray(proj(model.predict(lx, krtimes(lu, lx)))).flatten())
            sess.put_state(step + 1, np.asarray(lift(xs[step + 1]), dtype=np.complex128).reshape(1, -1))
            if streaming:                                                                      # mpc.py:281-285
                lu = wrapped.lift_u(u.reshape(-1, 1))
                lx = np.asarray(lift(xs[step])).reshape(-1, 1)
                model.fit_iteration(np.asarray(lift(xs[step + 1])).reshape(-1, 1), lx, krtimes(lu, lx))
            if exit_condition is not None and exit_condition(xs[step + 1], xs[step], us[step]):
                code = 1
                break
        if code == 0:
            clock.set_endsim(step + 1)
            return [np.vstack(xs[:step + 2]).T, np.vstack(us[:step + 1]).T], model, code
        clock.set_endsim(step)
        if step == 0:
            return [np.vstack(xs[:1]).T, None], model, code
        return [np.vstack(xs[:step + 1]).T, np.vstack(us[:step]).T], model, code
    finally:
        sess.close()


class _HeldControl:
    """interp1d(ts, us, kind='previous', fill_value='extrapolate') for the held control of one step."""

    def __init__(self, ts, us):
        self.x = np.asarray(ts)
        self.y = np.asarray(us)

    def __call__(self, t):
        idx = np.clip(np.searchsorted(self.x, t, side='right') - 1, 0, len(self.x) - 1)
        return self.y[..., idx]


def check_batch_exit(cond, B, n, plant_kind, where):
    """The batched entry points take None or a QuadraticExit that fits the ensemble: TypeError / ValueError before any device call."""
    require_device_exit(cond, where)
    if cond is not None:
        cond.check(B, n)
        if plant_kind == _lib.PLANT_NONE:
            raise ValueError("%s: an exit condition needs a device plant (with PLANT_NONE the host supplies the states)" % where)


def open_session(x0, models, dim_u, order, X_targ, U_targ, clock, plant_op0, plant_ops, Q, R, Qf, sat, du=None,
                 max_iter=100, warm_start=True, qp_flags=None, plant_kind=_lib.PLANT_HAMILTONIAN, device=-1,
                 force_complex=False, exact_qp=False, traceless=True, tile=None, generators=None, scales=None,
                 shared_generators=None, exit_condition=None, noise=None, observe=None):
    """An EnsembleSession loaded with mpc_batch's arguments (everything resident in HBM, nothing run yet).
    models = None with generators [1+m, n, n] (or [B, 1+m, n, n]) and optional scales [B, 1+m]: the members' models are built on the
    device (discretize_homogeneous of the scaled generators, vectorize.py:8-49), and a set of SHARED generators at order 1 lets the
    closed loop run on them directly where that kernel exists (d = 4; EnsembleSession(shared_generators=...)).
    exit_condition: None or a QuadraticExit the kernel evaluates for every member (EnsembleSession.set_exit_condition).
    noise: None or a MeasurementNoise the kernel adds to every measured state (EnsembleSession.set_noise).
    observe: None, or an observation kind (observe.py: OBSERVE_PARTIAL_TRACE, OBSERVE_QUBIT_BLOCK) for an observed plant: x0 is then
    the plant states [B, n_p], plant_op0 / plant_ops the plant's d_p x d_p operators (shared or per member), plant_kind stays at its
    default, the X0 field is observe_batch(observe, x0) and the loop runs with run_observed (EnsembleSession.set_observed_plant)."""
    x0 = np.ascontiguousarray(x0, dtype=np.complex128)
    if x0.ndim != 2:
        raise ValueError("open_session: x0 must have shape (B, n), got %s" % (x0.shape,))
    Bn, n = x0.shape
    z0 = None
    if observe is not None:
        # every shape is checked here, before the library is touched
        n = observe_dims(observe)[1]
        if plant_kind != _lib.PLANT_HAMILTONIAN:
            raise ValueError("open_session: with observe= the plant is the observed (Hamiltonian) plant: leave plant_kind at its default")
        if getattr(clock, "measure_freq", 1) != 1:
            raise ValueError("open_session: an observed plant is measured at every step (measure_freq=%d)" % clock.measure_freq)
        if exit_condition is not None or noise is not None:
            raise ValueError("open_session: exit conditions and measurement noise are not evaluated on the device for observed plants")
        plant_op0, plant_ops, _, z0 = check_observed_plant(observe, Bn, n, dim_u, plant_op0, plant_ops, x0, "open_session")
        plant_kind = _lib.PLANT_NONE
    check_batch_exit(exit_condition, Bn, n, plant_kind, "open_session")
    check_batch_noise(noise, Bn, n, plant_kind, "open_session")
    if models is None:
        if generators is None:
            raise TypeError("models is None: pass generators (and scales) to have the models built on the device")
        per_model = True
    else:
        models = np.asarray(models, dtype=np.complex128)
        if models.ndim == 2:
            models = models[None]
        per_model = models.shape[0] > 1
    op0 = np.asarray(plant_op0, dtype=np.complex128)
    ops = np.asarray(plant_ops, dtype=np.complex128)
    if op0.ndim == 2:
        op0 = op0[None]
    if ops.ndim == 3:
        ops = ops[None]
    per_plant = z0 is None and (op0.shape[0] > 1 or ops.shape[0] > 1)        # (an observed plant's operators are not session fields)
    if per_plant:
        op0 = np.broadcast_to(op0, (Bn,) + op0.shape[1:])
        ops = np.broadcast_to(ops, (Bn,) + ops.shape[1:])
    X_targ = np.asarray(X_targ)
    per_targ = X_targ.ndim == 3
    T, ns = clock.horizon, clock.n_steps
    cols = min(X_targ.shape[-1], ns + T + 1)
    sess = EnsembleSession(Bn, n, dim_u, order, T, ns, clock.dt, sat, du, max_iter, warm_start, qp_flags, plant_kind,
                           per_model, per_plant, per_targ, cols, device=device, force_complex=force_complex, traceless=traceless, tile=tile,
                           measure_freq=getattr(clock, "measure_freq", 1), exact_qp=exact_qp, shared_generators=shared_generators)
    try:
        if models is None:
            sess.build_models(clock.dt, generators, scales)
        sess.load_problem(models, x0 if z0 is None else observe_batch(observe, z0), X_targ, U_targ, Q, R, Qf, op0, ops)
        if z0 is not None:
            sess.set_observed_plant(observe, plant_op0, plant_ops, z0)
        if exit_condition is not None:
            sess.set_exit_condition(exit_condition)
        if noise is not None:
            sess.set_noise(noise)
    except Exception:
        sess.close()
        raise
    return sess


def mpc_batch(x0, models, dim_u, order, X_targ, U_targ, clock, plant_op0, plant_ops, Q, R, Qf, sat, du=None,
              max_iter=100, warm_start=True, qp_flags=None, plant_kind=_lib.PLANT_HAMILTONIAN, device=-1,
              force_complex=False, exact_qp=False, traceless=True, tile=None, generators=None, scales=None, shared_generators=None,
              exit_condition=None, noise=None, observe=None):
    """B independent closed loops in one launch.
    x0 [B, n]; models [B|1, n, n(1+P)] (or None with generators / scales: built on the device, see open_session);
    X_targ (n, cols) / U_targ (m, cols) shared (or [B, ...] each);
    plant_op0 [B|1, k, k], plant_ops [B|1, m, k, k] (k = d; plant_kind=_lib.PLANT_PROCESS: x0 and the targets are process vectors
    of n = d^4 entries and k = d, the gate's Hamiltonians - that plant always runs the complex path).  Returns a dict: xs [B, n, n_steps+1], us [B, m, n_steps]
    (entries beyond steps_done are not meaningful), exit_codes, steps_done, qp_solves [B, n_steps].
    exit_condition: None or a QuadraticExit, evaluated on the device; a member it stops has exit code 1 and steps_done = the step
    after which it fired (that step's entries are dropped, as mpc() drops them).
    noise: None or a MeasurementNoise: measurement noise drawn on the device for every member and measured step (kind "iid" runs
    the complex path); member b of this call is member noise.member_base + b of the generator.
    observe: None or an observation kind for an observed plant (open_session): x0 holds the plant states [B, n_p]; the loop stays
    on the device, two launches per step; the dict gains "zs" [B, n_p, n_steps+1], the plant states, and "xs" holds the observed
    states the QPs saw."""
    sess = open_session(x0, models, dim_u, order, X_targ, U_targ, clock, plant_op0, plant_ops, Q, R, Qf, sat, du, max_iter,
                        warm_start, qp_flags, plant_kind, device, force_complex, exact_qp, traceless, tile, generators, scales,
                        shared_generators, exit_condition, noise, observe)
    try:
        if observe is not None:
            sess.run_observed(0, clock.n_steps)
        else:
            sess.run(0, clock.n_steps)
        res = sess.results()
        if observe is not None:
            res["zs"] = np.swapaxes(sess.plant_states(), 1, 2)
        res["path"] = sess.path()
        res["path_detail"] = sess.path_detail()
        res["kernel_ms"] = sess.kernel_ms()[0]
        res["qp_stats"] = sess.qp_stats()
    finally:
        sess.close()
    res["xs"] = np.swapaxes(res["xs"], 1, 2)
    res["us"] = np.swapaxes(res["us"], 1, 2)
    return res

"""Resident ensemble session: thin object wrapper over the m4q_session_* C ABI (include/m4q.h).
All inputs live in HBM; `run` enqueues the fused closed-loop kernel on the session's stream."""
import ctypes as C

import numpy as np

from . import _lib
from .exit_condition import require_device_exit
from .noise import check_batch_noise
from .observe import check_observed_plant, observe_dims

_DTYPES = {
    _lib.F_MODELS: np.complex128, _lib.F_X0: np.complex128, _lib.F_X_TARG: np.complex128, _lib.F_U_TARG: np.float64,
    _lib.F_Q: np.complex128, _lib.F_R: np.complex128, _lib.F_QF: np.complex128, _lib.F_OP0: np.complex128,
    _lib.F_OPS: np.complex128, _lib.F_XS: np.complex128, _lib.F_US: np.float64, _lib.F_CODES: np.int32,
    _lib.F_STEPS_DONE: np.int32, _lib.F_QP_SOLVES: np.int32, _lib.F_X_GUESS: np.complex128, _lib.F_U_GUESS: np.float64,
}


def check_build_models_shapes(B, dim_x, dim_u, generators, scales):
    """The shapes m4q_session_build_models reads: generators [1+m, n, n], [1, 1+m, n, n] or [B, 1+m, n, n]; scales None or
    [B, 1+m].  The C side takes the sizes from the session, not from the arrays: anything else would be read past its end."""
    g = np.shape(generators)
    k = 1 + int(dim_u)
    if not (g == (k, dim_x, dim_x) or (len(g) == 4 and g[1:] == (k, dim_x, dim_x) and g[0] in (1, B))):
        raise ValueError("generators must have shape (%d, %d, %d), (1, %d, %d, %d) or (%d, %d, %d, %d), got %s"
                         % (k, dim_x, dim_x, k, dim_x, dim_x, B, k, dim_x, dim_x, g))
    if scales is not None and np.shape(scales) != (B, k):
        raise ValueError("scales must have shape (%d, %d), got %s" % (B, k, np.shape(scales)))


class EnsembleSession:
    def __init__(self, B, dim_x, dim_u, order, horizon, n_steps, dt, sat, du=None, max_iter=100, warm_start=True,
                 qp_flags=None, plant_kind=_lib.PLANT_HAMILTONIAN, model_per_instance=False, plant_per_instance=False,
                 target_per_instance=False, target_cols=None, ls_tol=1e-4, device=-1, force_complex=False, measure_freq=1,
                 exact_qp=False, traceless=True, tile=None, shared_generators=None):
        """exact_qp: solve every QP of the loop to the box-constrained optimum (M4Q_QP_EXACT_BOX, what the reference's OSQP
        call converges to) instead of clipping the Riccati rollout."""
        if sat is None:
            raise TypeError("sat is required (the reference negates it unconditionally, optimize.py:43 / lqr.py:76)")
        p = _lib.Problem()
        p.dim_x, p.dim_u, p.order, p.horizon, p.n_steps = dim_x, dim_u, order, horizon, n_steps
        p.max_iter, p.warm_start = int(max_iter), int(bool(warm_start))
        p.qp_flags = int(qp_flags if qp_flags is not None else (_lib.QP_DU_BAND if du is not None else 0))
        if exact_qp:
            p.qp_flags |= _lib.QP_EXACT_BOX
        p.plant_kind = int(plant_kind)
        p.model_per_instance, p.plant_per_instance = int(model_per_instance), int(plant_per_instance)
        p.target_per_instance = int(target_per_instance)
        p.target_cols = int(target_cols if target_cols is not None else n_steps + horizon + 1)
        # traceless=False keeps a real-path session on its d*d coordinates (M4Q_OPT_NO_TRACELESS) instead of the d*d - 1 traceless ones
        # tile: None / True = the library's choice (the backward sweep on matrix-core tiles where that form is built: d = 2, 3 with an
        # order-1 model, whenever the target is constant over the window), False = DPP sweeps (M4Q_OPT_NO_TILE)
        # shared_generators: None / True = the library's choice (models built by build_models from ONE generator set at order 1 run the
        # clipped traceless solve on the shared generators where that kernel is built: d = 4), False = per-member models (M4Q_OPT_NO_SG)
        p.reserved = (_lib.OPT_FORCE_COMPLEX if force_complex else 0) | (0 if traceless else _lib.OPT_NO_TRACELESS) | \
            (_lib.OPT_NO_TILE if tile is False else 0) | (_lib.OPT_NO_SG if shared_generators is False else 0)
        p.measure_freq = int(measure_freq)
        p.dt, p.sat, p.du, p.ls_tol = float(dt), float(sat), float(du if du is not None else 0.0), float(ls_tol)
        self.problem = p
        self.B = int(B)
        self._h = C.c_void_p()
        self._L = _lib.lib()
        _lib.check(self._L.m4q_session_create(C.byref(p), self.B, int(device), C.byref(self._h)))
        self._keep = {}
        self.observe = 0              # the observation kind once set_observed_plant has been called

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.m4q_session_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def field_bytes(self, field):
        return int(self._L.m4q_session_field_bytes(self._h, field))

    def upload(self, field, array):
        a = np.ascontiguousarray(array, dtype=_DTYPES[field])
        if a.nbytes != self.field_bytes(field):
            raise ValueError("field %d expects %d bytes, array has %d (shape %s)" % (field, self.field_bytes(field), a.nbytes,
                                                                                      a.shape))
        _lib.check(self._L.m4q_session_upload(self._h, field, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, field, shape):
        out = np.empty(shape, dtype=_DTYPES[field])
        _lib.check(self._L.m4q_session_download(self._h, field, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def put_state(self, step, x):
        a = np.ascontiguousarray(x, dtype=np.complex128).reshape(self.B, self.problem.dim_x)
        _lib.check(self._L.m4q_session_put_state(self._h, int(step), a.ctypes.data_as(C.c_void_p)))

    def get_state(self, step):
        out = np.empty((self.B, self.problem.dim_x), dtype=np.complex128)
        _lib.check(self._L.m4q_session_get_state(self._h, int(step), out.ctypes.data_as(C.c_void_p)))
        return out

    def device_ptr(self, field):
        return self._L.m4q_session_device_ptr(self._h, field)

    def bind_output(self, field, device_ptr, nbytes):
        _lib.check(self._L.m4q_session_bind_output(self._h, field, C.c_void_p(device_ptr), nbytes))

    def copy_final_state(self, device_ptr):
        """xs[:, n_steps, :] -> device memory [B][n] complex, on the session stream (final-state-only gather buffers)."""
        _lib.check(self._L.m4q_session_copy_final_state(self._h, C.c_void_p(device_ptr)))

    def copy_status(self, device_ptr):
        """the launch's watchdog flag -> one int32 of device memory, on the session stream (a gather buffer's status word)."""
        _lib.check(self._L.m4q_session_copy_status(self._h, C.c_void_p(device_ptr)))

    def build_models(self, dt, generators, scales=None):
        """Fill the MODELS field on the device: generators [1+m, n, n] (shared) or [B, 1+m, n, n], scales [B, 1+m]."""
        check_build_models_shapes(self.B, self.problem.dim_x, self.problem.dim_u, generators, scales)
        g = np.ascontiguousarray(generators, dtype=np.complex128)
        per = 1 if g.ndim == 4 and g.shape[0] > 1 else 0
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
        _lib.check(self._L.m4q_session_build_models(self._h, float(dt), g.ctypes.data_as(_lib._dp), per,
                                                    sc.ctypes.data_as(_lib._dp) if sc is not None else None))

    def set_exit_condition(self, cond):
        """Have the kernel end each member with exit code 1 once its QuadraticExit fires (m4q_session_set_exit); None clears it.
        Applies to the launches that follow; needs a device plant."""
        L = self._L
        if cond is None:
            _lib.check(L.m4q_session_set_exit(self._h, 0, None, None, 0, None, 0))
            return
        require_device_exit(cond, "EnsembleSession.set_exit_condition")
        cond.check(self.B, self.problem.dim_x)
        W = np.ascontiguousarray(cond.W, dtype=np.complex128)
        f = np.ascontiguousarray(cond.target, dtype=np.complex128)
        thr = np.ascontiguousarray(cond.thr, dtype=np.float64).reshape(-1)
        _lib.check(L.m4q_session_set_exit(self._h, cond.mode, W.ctypes.data_as(_lib._dp), f.ctypes.data_as(_lib._dp),
                                          int(f.ndim == 2), thr.ctypes.data_as(_lib._dp), int(cond.thr.ndim == 1)))

    def set_noise(self, noise):
        """Have the kernel add a MeasurementNoise to every measured state before it is stored (m4q_session_set_noise); None clears
        it.  Set it before the first run: later calls may change sigma, seed and member_base, not the kind.  Needs a device plant;
        kind "iid" runs the complex path.  Like the exit condition it is a setting of the session, not part of state(): a
        checkpoint restored into a fresh session continues the same run once that session is given the same noise."""
        if noise is None:
            _lib.check(self._L.m4q_session_set_noise(self._h, 0, None, 0, 0, 0))
            return
        check_batch_noise(noise, self.B, self.problem.dim_x, self.problem.plant_kind, "EnsembleSession.set_noise")
        sg = np.ascontiguousarray(noise.sigma, dtype=np.float64).reshape(-1)
        _lib.check(self._L.m4q_session_set_noise(self._h, noise.mode, sg.ctypes.data_as(_lib._dp), int(noise.sigma.ndim == 1),
                                                 noise.seed, noise.member_base))

    def run(self, step_begin=0, step_end=None):
        _lib.check(self._L.m4q_session_run(self._h, int(step_begin), int(self.problem.n_steps if step_end is None else step_end)))

    def set_observed_plant(self, kind, op0, ops, z0):
        """Give a PLANT_NONE session an observed plant (observe.py; m4q_session_set_observed_plant): plant states z0 [B, n_p] that
        evolve by the Hamiltonian plant's arithmetic under op0 [B|1, d_p, d_p] and ops [B|1, m, d_p, d_p], and the loop state
        x = observe(z).  Writes zs[:, 0] = z0 and xs[:, 0] = observe(z0); the X0 field is the caller's (observe_batch(kind, z0):
        load_problem).  Before the first run, measure_freq 1.  Every shape is checked here, before the library is touched."""
        p = self.problem
        if p.plant_kind != _lib.PLANT_NONE:
            raise ValueError("EnsembleSession.set_observed_plant: the session has a device plant (plant_kind=%d); an observed plant "
                             "is a setting of a PLANT_NONE session" % p.plant_kind)
        if p.measure_freq > 1:
            raise ValueError("EnsembleSession.set_observed_plant: measure_freq=%d; an observed plant is measured at every step"
                             % p.measure_freq)
        op0, ops, per, z0 = check_observed_plant(kind, self.B, p.dim_x, p.dim_u, op0, ops, z0, "EnsembleSession.set_observed_plant")
        _lib.check(self._L.m4q_session_set_observed_plant(self._h, int(kind), op0.ctypes.data_as(_lib._dp), ops.ctypes.data_as(_lib._dp),
                                                          per, z0.ctypes.data_as(_lib._dp)))
        self.observe = int(kind)

    def _need_observed(self, where):
        if not self.observe:
            raise ValueError("EnsembleSession.%s: no observed plant is set (set_observed_plant)" % where)

    def run_observed(self, step_begin=0, step_end=None):
        """run() for a session with an observed plant (m4q_session_run_observed): for every step of the range one MPC launch, then
        the kernel that advances the plant and writes the observed state into xs[:, step + 1], all on the session's stream with no
        host round trip in between."""
        self._need_observed("run_observed")
        _lib.check(self._L.m4q_session_run_observed(self._h, int(step_begin),
                                                    int(self.problem.n_steps if step_end is None else step_end)))

    def plant_states(self):
        """zs [B, n_steps + 1, n_p]: the plant states of a session with an observed plant (columns beyond steps_done are zero)."""
        self._need_observed("plant_states")
        out = np.empty((self.B, self.problem.n_steps + 1, observe_dims(self.observe)[0]), dtype=np.complex128)
        _lib.check(self._L.m4q_session_plant_states(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def put_plant_states(self, zs):
        """Inverse of plant_states() (restore)."""
        self._need_observed("put_plant_states")
        shape = (self.B, self.problem.n_steps + 1, observe_dims(self.observe)[0])
        a = np.ascontiguousarray(zs, dtype=np.complex128)
        if a.shape != shape:
            raise ValueError("EnsembleSession.put_plant_states: zs must have shape %s, got %s" % (shape, a.shape))
        _lib.check(self._L.m4q_session_put_plant_states(self._h, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def sync(self):
        _lib.check(self._L.m4q_session_sync(self._h))

    def set_codes(self, codes):
        a = np.ascontiguousarray(codes, dtype=np.int32)
        _lib.check(self._L.m4q_session_set_codes(self._h, a.ctypes.data_as(_lib._ip)))

    def kernel_ms(self):
        ms = C.c_double()
        n = C.c_int32()
        _lib.check(self._L.m4q_session_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def qp_stats(self):
        """exact_qp sessions: (QP solves, pinned Riccati sweeps, ratio-test steps, solves ended by KKT / at working
        precision / by the iteration cap) of the last launch."""
        out = (C.c_int64 * 6)()
        _lib.check(self._L.m4q_session_qp_stats(self._h, out))
        return tuple(int(v) for v in out)

    def path(self):
        """'real' if the uploaded problem runs in a Hermitian operator basis with real arithmetic, else 'complex'."""
        return "real" if _lib.check(self._L.m4q_session_path(self._h)) >= 1 else "complex"

    def path_detail(self):
        """'complex', 'real' (d*d Hermitian coordinates), 'traceless' (the d*d - 1 traceless Hermitian coordinates) or
        'traceless-tile' (the same with the backward sweep of the clipped solve / the pinned sweep of the exact solve on fp64
        matrix-core tiles), or 'traceless-sg' (the traceless clipped solve on shared generators and per-member scales)."""
        return ("complex", "real", "traceless", "traceless-tile", "traceless-sg")[_lib.check(self._L.m4q_session_path(self._h))]

    def info(self):
        hbm = C.c_int64()
        grid = C.c_int32()
        lds = C.c_int32()
        _lib.check(self._L.m4q_session_info(self._h, C.byref(hbm), C.byref(grid), C.byref(lds)))
        return {"hbm_bytes": hbm.value, "grid": grid.value, "lds_bytes": lds.value}

    # ---- convenience ----
    def load_problem(self, models, x0, X_targ, U_targ, Q, R, Qf, op0=None, ops=None):
        """Reference-shaped inputs: X_targ (n, cols) / U_targ (m, cols) (or with a leading ensemble
        axis), models [B|1, n, n(1+P)] (or [n, n(1+P)])."""
        p = self.problem
        n, m, cols = p.dim_x, p.dim_u, p.target_cols
        if models is not None:                       # None: already built on the device (build_models)
            self.upload(_lib.F_MODELS, models)
        self.upload(_lib.F_X0, x0)
        Xt = np.asarray(X_targ, dtype=np.complex128)
        Ut = np.real(np.asarray(U_targ)).astype(np.float64)
        Ut_full = np.zeros(Xt.shape[:-2] + (m, cols))
        Ut_full[..., :min(cols, Ut.shape[-1])] = Ut[..., :cols]
        self.upload(_lib.F_X_TARG, np.swapaxes(Xt[..., :cols], -1, -2))
        self.upload(_lib.F_U_TARG, np.swapaxes(Ut_full, -1, -2))
        self.upload(_lib.F_Q, np.asarray(Q, dtype=np.complex128).reshape(n, n))
        self.upload(_lib.F_R, np.asarray(R, dtype=np.complex128).reshape(m, m))
        self.upload(_lib.F_QF, np.asarray(Qf, dtype=np.complex128).reshape(n, n))
        if p.plant_kind != _lib.PLANT_NONE:
            self.upload(_lib.F_OP0, op0)
            self.upload(_lib.F_OPS, ops)

    def state(self):
        """Everything a run needs to resume at MPC step k (checkpoint): states, controls, SQP guesses, codes - and the plant states
        "zs" of a session with an observed plant (only then)."""
        p = self.problem
        B, n, m, ns, T = self.B, p.dim_x, p.dim_u, p.n_steps, p.horizon
        st = {
            "xs": self.download(_lib.F_XS, (B, ns + 1, n)), "us": self.download(_lib.F_US, (B, ns, m)),
            "x_guess": self.download(_lib.F_X_GUESS, (B, T + 1, n)), "u_guess": self.download(_lib.F_U_GUESS, (B, T, m)),
            "exit_codes": self.download(_lib.F_CODES, (B,)), "steps_done": self.download(_lib.F_STEPS_DONE, (B,)),
        }
        if self.observe:
            st["zs"] = self.plant_states()
        return st

    def restore(self, state):
        """Inverse of state(): afterwards run(k, ...) continues a run interrupted before step k.  A session with an observed plant
        (set_observed_plant first: the operators are a setting, not part of the state) takes the plant states "zs" too."""
        if self.observe:
            self.put_plant_states(state["zs"])
        self.upload(_lib.F_XS, state["xs"])
        self.upload(_lib.F_US, state["us"])
        self.upload(_lib.F_X_GUESS, state["x_guess"])
        self.upload(_lib.F_U_GUESS, state["u_guess"])
        self.upload(_lib.F_STEPS_DONE, state["steps_done"])
        self.set_codes(state["exit_codes"])

    def results(self):
        p = self.problem
        B, n, m, ns = self.B, p.dim_x, p.dim_u, p.n_steps
        return {
            "xs": self.download(_lib.F_XS, (B, ns + 1, n)),
            "us": self.download(_lib.F_US, (B, ns, m)),
            "exit_codes": self.download(_lib.F_CODES, (B,)),
            "steps_done": self.download(_lib.F_STEPS_DONE, (B,)),
            "qp_solves": self.download(_lib.F_QP_SOLVES, (B, ns)),
        }

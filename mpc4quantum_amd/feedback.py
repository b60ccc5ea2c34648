"""A stored feedback law run on a whole ensemble of plants or models in ONE launch (m4q_plant_feedback_batch,
m4q_model_feedback_batch): the tier between the open-loop rollouts (rollout.py), which do not react to the plant, and mpc_batch,
which re-solves a QP at every step - time-varying gains around a nominal trajectory (TVLQR) with saturation, a slew band and
measurement noise, the controller an MPC run designs once and cheap hardware then runs.

The definitions are here, in NumPy and SciPy (no torch, no device call).  A law is the `Gains` of lqr.py:61 as quad_program_batch
returns them, gains[t][col][k] with col = n the affine column, around x_ref[t] and u_ref[t].  Step t of member b in state x_t:
    s_k  = sum_j Re(K_t[j][k] (x_t - x_ref[t])_j) + Re(K_t[n][k]) + u_ref[t][k]
    lo   = -sat, hi = sat;  with a band  lo = max(lo, p_k - du), hi = min(hi, p_k + du),  p = u_prev[b] at t = 0, then u_{t-1}
    u_t[k] = min(max(s_k, lo), hi)       (lo > hi: hi wins - the order of lqr.py:74-76 as rollout_forward evaluates it)
    x_{t+1} = step(x_t, u_scale[b] * u_t, dts[t])  (+ noise.sample([b], t + 1, n): stored, seen by the next control, stepped from)
min and max are C's fmin and fmax (np.fmin, np.fmax): against a NaN s_k they return the bound, so a member whose state is lost
commands finite controls where its bounds are finite; `status` is what reports it.

Arrays keep the ensemble axis outermost, as the C ABI lays them out.  Every shape and value is checked, and ValueError or TypeError
raised, before the library is touched."""
import numpy as np

from . import _lib
from .grad import _models
from .library import create_power_list
from .noise import require_noise
from .rollout import _common, _outputs, _plant_operators, _ptr, dts_of

_ip = _lib._ip


class FeedbackLaw:
    """u_t = clip(Re(K_t [x_t - x_ref[t] ; 1]) + u_ref[t]).

    gains [N, n + 1, m] or [B, N, n + 1, m] complex (quad_program_batch's layout); x_ref [N, n] or [B, N, n] complex (an array of
    N + 1 rows is accepted, its last row ignored); u_ref [N, m] or [B, N, m] real: all three shared by the ensemble or all three
    per member.  sat > 0 (inf: no box).  du: None, or > 0 and finite - then u_prev [m] or [B, m] is required."""

    def __init__(self, gains, x_ref, u_ref, sat, du=None, u_prev=None):
        gains = np.ascontiguousarray(gains, dtype=np.complex128)
        x_ref = np.asarray(x_ref, dtype=np.complex128)
        u_ref = np.asarray(u_ref)
        if np.iscomplexobj(u_ref):
            raise TypeError("u_ref must be real")
        u_ref = np.ascontiguousarray(u_ref, dtype=np.float64)
        if gains.ndim not in (3, 4) or gains.shape[-3] < 1 or gains.shape[-2] < 2 or gains.shape[-1] < 1:
            raise ValueError("gains must be [N, n + 1, m] or [B, N, n + 1, m], got shape %s" % (gains.shape,))
        per = gains.ndim == 4
        N, n1, m = gains.shape[-3:]
        n = n1 - 1
        lead = gains.shape[:1] if per else ()
        if x_ref.shape not in (lead + (N, n), lead + (N + 1, n)):
            raise ValueError("x_ref must be %s (or with N + 1 rows) beside gains %s, got %s" % (lead + (N, n), gains.shape, x_ref.shape))
        if u_ref.shape != lead + (N, m):
            raise ValueError("u_ref must be %s beside gains %s, got %s" % (lead + (N, m), gains.shape, u_ref.shape))
        if per and lead[0] < 1:
            raise ValueError("a per-member law needs at least one member")
        sat = float(sat)
        if not sat > 0:
            raise ValueError("sat must be positive (inf: no box), got %r" % (sat,))
        if du is not None:
            du = float(du)
            if not (du > 0 and np.isfinite(du)):
                raise ValueError("du must be positive and finite (or None), got %r" % (du,))
            if u_prev is None:
                raise ValueError("a band (du) needs u_prev, the control applied before step 0")
        if u_prev is not None:
            u_prev = np.ascontiguousarray(u_prev, dtype=np.float64)
            if u_prev.ndim not in (1, 2) or u_prev.shape[-1] != m or (u_prev.ndim == 2 and u_prev.shape[0] < 1):
                raise ValueError("u_prev must be [m] or [B, m] with m = %d, got %s" % (m, u_prev.shape))
        self.gains = gains
        self.x_ref = np.ascontiguousarray(x_ref[..., :N, :])
        self.u_ref = u_ref
        self.sat, self.du, self.u_prev = sat, du, u_prev
        self.N, self.n, self.m = N, n, m

    @property
    def members(self):
        """B if the law is per member, else None."""
        return self.gains.shape[0] if self.gains.ndim == 4 else None

    @property
    def prev_members(self):
        """B if u_prev is per member, else None."""
        return self.u_prev.shape[0] if (self.u_prev is not None and self.u_prev.ndim == 2) else None

    def check(self, B, n):
        """ValueError unless the law fits an ensemble of B members with n-dimensional states."""
        if n != self.n:
            raise ValueError("the law is for states of %d entries, the ensemble's have %d" % (self.n, n))
        for what, have in (("gains", self.members), ("u_prev", self.prev_members)):
            if have is not None and have != B:
                raise ValueError("the law has %s for %d members, the ensemble has %d" % (what, have, B))

    def prev(self, member=0):
        """p at t = 0 for `member`: its u_prev, zeros when there is none."""
        if self.u_prev is None:
            return np.zeros(self.m)
        return self.u_prev[member] if self.u_prev.ndim == 2 else self.u_prev

    def terms(self, t, x, p=None, member=0):
        """(u, s, lo, hi), each [m], of step t for one member in state x; p [m]: the control applied before (read with a band)."""
        b = member if self.members is not None else ()
        K, xb, ub = self.gains[b][t], self.x_ref[b][t], self.u_ref[b][t]
        d = np.asarray(x, dtype=np.complex128).reshape(self.n) - xb
        s = np.real(K[:self.n].T @ d) + np.real(K[self.n]) + ub
        lo, hi = np.full(self.m, -self.sat), np.full(self.m, self.sat)
        if self.du is not None:
            p = self.prev(member) if p is None else np.asarray(p, dtype=np.float64).reshape(self.m)
            lo, hi = np.fmax(lo, p - self.du), np.fmin(hi, p + self.du)
        return np.fmin(np.fmax(s, lo), hi), s, lo, hi

    def control(self, t, x, p=None, member=0):
        """u_t [m] for one member in state x (the formula of the module's docstring)."""
        return self.terms(t, x, p, member)[0]

    @classmethod
    def from_quad_program(cls, gains, X_bm, U_bm, sat, du=None, u_prev=None):
        """The law one quad_program_batch solve leaves behind: its gains [B, T, n + 1, m] (or one member's [T, n + 1, m]) around the
        benchmark trajectories it was given, X_bm [B|1, T + 1, n] or [T + 1, n] and U_bm [B|1, T, m] or [T, m]."""
        gains = np.asarray(gains)
        X_bm, U_bm = np.asarray(X_bm), np.real(np.asarray(U_bm))
        if gains.ndim == 4:                       # per member: a benchmark shared by the solve is repeated
            Bn = gains.shape[0]
            X_bm = np.broadcast_to(X_bm if X_bm.ndim == 3 else X_bm[None], (Bn,) + X_bm.shape[-2:])
            U_bm = np.broadcast_to(U_bm if U_bm.ndim == 3 else U_bm[None], (Bn,) + U_bm.shape[-2:])
        else:
            X_bm = X_bm[0] if X_bm.ndim == 3 else X_bm
            U_bm = U_bm[0] if U_bm.ndim == 3 else U_bm
        return cls(gains, X_bm, U_bm, sat, du, u_prev)

    @classmethod
    def along_trajectory(cls, model, order, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du=None, u_prev=None, exact=False):
        """TVLQR around a nominal trajectory (for instance the xs, us of an MPC run): the model [n, n (1 + P)] (DMDc.A's layout)
        linearised along X_nom [N + 1, n] (or [N, n]), U_nom [N, m] with linearize_batch, ONE quad_program_batch from X_nom[0]
        towards X_targ [N + 1, n], U_targ [N, m] under Q_ls [N + 1, n, n] (or [n, n]) and R_ls [N, m, m] (or [m, m]), and its
        gains wrapped.  sat, du, u_prev: the QP's bounds, and the law's."""
        from .linearize import WrapModel
        from .optimize import quad_program_batch
        X_nom = np.asarray(X_nom, dtype=np.complex128)
        U_nom = np.ascontiguousarray(np.real(np.asarray(U_nom)), dtype=np.float64)
        if U_nom.ndim != 2 or X_nom.ndim != 2 or X_nom.shape[0] not in (U_nom.shape[0], U_nom.shape[0] + 1):
            raise ValueError("X_nom must be [N + 1, n] (or [N, n]) and U_nom [N, m], got %s and %s" % (X_nom.shape, U_nom.shape))
        N, m = U_nom.shape
        n = X_nom.shape[1]
        model = np.asarray(model, dtype=np.complex128)
        if model.ndim != 2 or model.shape[0] != n or model.shape[1] % n:
            raise ValueError("model must be [n, n (1 + P)] with n = %d, got %s" % (n, model.shape))
        X_targ = np.asarray(X_targ, dtype=np.complex128)
        U_targ = np.real(np.asarray(U_targ)).astype(np.float64)
        if X_targ.shape != (N + 1, n) or U_targ.shape != (N, m):
            raise ValueError("X_targ must be [N + 1, n] = (%d, %d) and U_targ [N, m] = (%d, %d), got %s and %s"
                             % (N + 1, n, N, m, X_targ.shape, U_targ.shape))
        Q_ls, R_ls = np.asarray(Q_ls, dtype=np.complex128), np.asarray(R_ls, dtype=np.complex128)
        if Q_ls.shape == (n, n):
            Q_ls = np.broadcast_to(Q_ls, (N + 1, n, n))
        if R_ls.shape == (m, m):
            R_ls = np.broadcast_to(R_ls, (N, m, m))
        if Q_ls.shape != (N + 1, n, n) or R_ls.shape != (N, m, m):
            raise ValueError("Q_ls must be [N + 1, n, n] or [n, n] and R_ls [N, m, m] or [m, m], got %s and %s" % (Q_ls.shape, R_ls.shape))
        law = cls(np.zeros((N, n + 1, m)), X_targ, U_targ, sat, du, u_prev)          # (the law's own checks, before the library)
        if law.prev_members is not None:
            raise ValueError("along_trajectory solves one QP: u_prev must be [m]")
        wm = WrapModel(model[:, :n], model[:, n:], m, int(order))
        A_ls, B_ls, D_ls = wm.linearize_batch(X_nom[None, :N], U_nom[None])
        _, _, _, gains = quad_program_batch(X_nom[:1], X_targ[None], U_targ[None], Q_ls, R_ls, A_ls, B_ls, D_ls,
                                            None if (u_prev is None or du is None) else law.u_prev[None], sat, du, exact=exact)
        return cls.from_quad_program(gains[0], X_targ, U_targ, sat, du, u_prev)

    @classmethod
    def along_plant_trajectory(cls, op0, ops, dt_or_ts, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du=None, u_prev=None,
                               kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False):
        """The plant-side twin of along_trajectory: TVLQR around nominal trajectories with the PLANT's own Jacobians - one
        plant_linearize_batch (the exact linearisation of the step the law will run on), one quad_program_batch, the gains wrapped.

        op0, ops, dt_or_ts, kind, u_scale as plant_linearize_batch.  One nominal, X_nom [N + 1, n] (or [N, n]) and U_nom [N, m],
        gives one law, as along_trajectory; per-member nominals X_nom [B, N + 1, n] (or [B, N, n]), U_nom [B, N, m] - for instance
        the xs, us of a finished mpc_batch run - give a per-member law, with per-member operators, u_scale [B, m] and u_prev [B, m]
        where given.  X_targ [N + 1, n] and U_targ [N, m], shared or with a leading B; Q_ls, R_ls, sat, du, exact as
        along_trajectory.  The Jacobians pass through the host between the two launches (along_plant_trajectory_fused: they do not)."""
        return cls._plant_trajectory_law(False, op0, ops, dt_or_ts, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du, u_prev, kind, u_scale,
                                         exact)

    @classmethod
    def along_plant_trajectory_fused(cls, op0, ops, dt_or_ts, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du=None, u_prev=None,
                                     kind=_lib.PLANT_HAMILTONIAN, u_scale=None, exact=False):
        """along_plant_trajectory (same arguments, same checks, the same law within the project's tolerance) in ONE device call:
        plant_quad_program_batch, the linearisation and the QP with the Jacobians left on the device."""
        return cls._plant_trajectory_law(True, op0, ops, dt_or_ts, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du, u_prev, kind, u_scale,
                                         exact)

    @classmethod
    def _plant_trajectory_law(cls, fused, op0, ops, dt_or_ts, X_nom, U_nom, X_targ, U_targ, Q_ls, R_ls, sat, du, u_prev, kind, u_scale,
                              exact):
        """along_plant_trajectory and along_plant_trajectory_fused: the checks, then the two calls or the one."""
        from .optimize import quad_program_batch
        from .plant_linearize import plant_linearize_batch, plant_quad_program_batch
        X_nom = np.asarray(X_nom, dtype=np.complex128)
        U_nom = np.asarray(U_nom)
        if np.iscomplexobj(U_nom):
            raise TypeError("U_nom must be real")
        U_nom = np.ascontiguousarray(U_nom, dtype=np.float64)
        per = X_nom.ndim == 3
        if X_nom.ndim not in (2, 3) or U_nom.ndim != X_nom.ndim or min(X_nom.shape) < 1 or min(U_nom.shape) < 1 \
                or X_nom.shape[-2] not in (U_nom.shape[-2], U_nom.shape[-2] + 1) or (per and X_nom.shape[0] != U_nom.shape[0]):
            raise ValueError("X_nom must be [N + 1, n] (or [N, n]) and U_nom [N, m], both with or both without a leading B, got %s "
                             "and %s" % (X_nom.shape, U_nom.shape))
        if not per:
            X_nom, U_nom = X_nom[None], U_nom[None]
        B, N, m = U_nom.shape
        n = X_nom.shape[2]
        X_targ = np.asarray(X_targ, dtype=np.complex128)
        U_targ = np.asarray(U_targ)
        if np.iscomplexobj(U_targ):
            raise TypeError("U_targ must be real")
        U_targ = np.asarray(U_targ, dtype=np.float64)
        lead = (B,) if per else ()
        if X_targ.shape not in ((N + 1, n), lead + (N + 1, n)) or U_targ.shape not in ((N, m), lead + (N, m)):
            raise ValueError("X_targ must be [N + 1, n] = (%d, %d) and U_targ [N, m] = (%d, %d), shared or with the nominal's leading "
                             "B, got %s and %s" % (N + 1, n, N, m, X_targ.shape, U_targ.shape))
        if X_targ.ndim == 3 or U_targ.ndim == 3:      # (the QP takes both per member or both shared)
            X_targ, U_targ = np.broadcast_to(X_targ, (B, N + 1, n)), np.broadcast_to(U_targ, (B, N, m))
        Q_ls, R_ls = np.asarray(Q_ls, dtype=np.complex128), np.asarray(R_ls, dtype=np.complex128)
        if Q_ls.shape == (n, n):
            Q_ls = np.broadcast_to(Q_ls, (N + 1, n, n))
        if R_ls.shape == (m, m):
            R_ls = np.broadcast_to(R_ls, (N, m, m))
        if Q_ls.shape != (N + 1, n, n) or R_ls.shape != (N, m, m):
            raise ValueError("Q_ls must be [N + 1, n, n] or [n, n] and R_ls [N, m, m] or [m, m], got %s and %s" % (Q_ls.shape, R_ls.shape))
        law = cls(np.zeros(lead + (N, n + 1, m)), np.broadcast_to(X_targ, lead + (N + 1, n)), np.broadcast_to(U_targ, lead + (N, m)),
                  sat, du, u_prev)                    # (the law's own checks, before the library)
        if law.prev_members is not None and not (per and law.prev_members == B):
            raise ValueError("u_prev must be [m]%s, got %s" % (" or [B, m] with B = %d" % B if per else " (one nominal: one QP)",
                                                               law.u_prev.shape))
        band = u_prev is not None and du is not None
        if fused:
            _, _, _, gains = plant_quad_program_batch(X_nom[:, :N], U_nom, op0, ops, dt_or_ts, X_targ.reshape(-1, N + 1, n),
                                                      U_targ.reshape(-1, N, m), Q_ls, R_ls, sat, du=du if band else None,
                                                      u_prev=np.broadcast_to(law.u_prev, (B, m)) if band else None, x_init=X_nom[:, 0],
                                                      kind=kind, u_scale=u_scale, exact=exact)
            return cls.from_quad_program(gains if per else gains[0], X_targ, U_targ, sat, du, u_prev)
        A_ls, B_ls, D_ls = plant_linearize_batch(X_nom[:, :N], U_nom, op0, ops, dt_or_ts, kind, u_scale)
        _, _, _, gains = quad_program_batch(X_nom[:, 0], X_targ.reshape(-1, N + 1, n), U_targ.reshape(-1, N, m), Q_ls, R_ls, A_ls, B_ls, D_ls,
                                            np.broadcast_to(law.u_prev, (B, m)) if band else None, sat, du, exact=exact)
        return cls.from_quad_program(gains if per else gains[0], X_targ, U_targ, sat, du, u_prev)


# ---------------------------------------------------------------- the definitions
def _plant_step(kind, x, v, op0, ops, dt):
    """One held-control step of the three device plants (SciPy's expm)."""
    from scipy.linalg import expm
    G = op0.astype(np.complex128)
    for k in range(len(v)):
        G = G + v[k] * ops[k]
    if kind == _lib.PLANT_GENERATOR:
        return expm(dt * G) @ x
    U = expm(-1j * dt * G)
    d = G.shape[0]
    if kind == _lib.PLANT_HAMILTONIAN:
        return (U @ x.reshape(d, d) @ U.conj().T).reshape(-1)
    return (np.kron(U, U.conj()) @ x.reshape(d * d, d * d)).reshape(-1)


def _model_step(model, powers, x, v):
    """x+ = A [x ; lift_u(v) (x) x] (model.py:81-93)."""
    n = x.shape[0]
    A = model[:, :n].astype(np.complex128)
    for p, e in enumerate(powers):
        A = A + float(np.prod(np.asarray(v, dtype=np.float64) ** np.asarray(e))) * model[:, (1 + p) * n:(2 + p) * n]
    return A @ x


def _check_noise(noise, B, n, hermitian_ok, where):
    require_noise(noise, where)
    if noise is None:
        return
    noise.check(B, n)
    if noise.kind == "hermitian" and not hermitian_ok:
        raise ValueError("%s: hermitian noise needs a density-matrix state; a process plant's is a process vector (use kind='iid')"
                         % where)


def _prepare(x0, law, u_scale, noise, W, target, keep, figure, hermitian_ok, where):
    """The checks and the layout the two feedback runs and their definitions share."""
    if not isinstance(law, FeedbackLaw):
        raise TypeError("%s takes a FeedbackLaw, not %r" % (where, type(law).__name__))
    x0, _, _, u_scale, W, target, t_per, xs_mode, q_mode = _common(x0, law.u_ref, u_scale, W, target, keep, figure, need_output=False)
    B, n = x0.shape
    law.check(B, n)
    _check_noise(noise, B, n, hermitian_ok, where)
    return x0, u_scale, W, target, t_per, xs_mode, q_mode


def _reference(step, x0, law, u_scale, noise, W, target, t_per, xs_mode, q_mode):
    B, n = x0.shape
    N, m = law.N, law.m
    xs = np.empty((B, N + 1, n), dtype=np.complex128)
    us = np.empty((B, N, m))
    clipped = np.zeros(B, dtype=np.int32)
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        x = xs[b, 0] = x0[b]
        p = law.prev(b)
        for t in range(N):
            u, s, lo, hi = law.terms(t, x, p, b)
            clipped[b] += int(np.count_nonzero((s <= lo) | (s >= hi)))
            x = step(b, t, x, sc * u)
            if noise is not None:
                x = x + noise.sample([b], t + 1, n)[0]
            xs[b, t + 1], us[b, t], p = x, u, u
    out = {}
    if xs_mode:
        out["xs"] = xs if xs_mode == 2 else np.ascontiguousarray(xs[:, N])
    if q_mode:
        d = xs - (target.reshape(-1, n)[:, None, :] if t_per else target.reshape(1, 1, n))
        q = np.einsum('btj,jk,btk->bt', d.conj(), W, d).real
        out["q"] = q if q_mode == 2 else np.ascontiguousarray(q[:, N])
    out["us"], out["clipped"] = us, clipped
    bad = ~np.isfinite(xs).all(axis=(1, 2)) | ~np.isfinite(us).all(axis=(1, 2))
    out["status"] = np.where(bad, 3, 0).astype(np.int32)
    return out


def plant_feedback_reference(x0, law, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, noise=None, W=None, target=None,
                             keep="all", figure="none"):
    """The definition of plant_feedback_batch (same arguments), on the host, member by member: returns "xs" and / or "q" as asked,
    and always "us" [B, N, m], "clipped" [B] and "status" [B]."""
    kind = int(kind)
    x0, u_scale, W, target, t_per, xs_mode, q_mode = _prepare(x0, law, u_scale, noise, W, target, keep, figure,
                                                               kind != _lib.PLANT_PROCESS, "plant_feedback_reference")
    B, n = x0.shape
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, law.m)
    dts = dts_of(dt_or_ts, law.N)
    k = op0.shape[-1]
    o0, ok = op0.reshape(-1, k, k), ops.reshape(-1, law.m, k, k)
    return _reference(lambda b, t, x, v: _plant_step(kind, x, v, o0[b if per else 0], ok[b if per else 0], dts[t]),
                      x0, law, u_scale, noise, W, target, t_per, xs_mode, q_mode)


def model_feedback_reference(x0, law, models, order, u_scale=None, noise=None, W=None, target=None, keep="all", figure="none"):
    """The definition of model_feedback_batch (same arguments), on the host."""
    x0, u_scale, W, target, t_per, xs_mode, q_mode = _prepare(x0, law, u_scale, noise, W, target, keep, figure, True,
                                                               "model_feedback_reference")
    B, n = x0.shape
    models, order, m_per = _models(models, order, B, n, law.m)
    powers = create_power_list(order, law.m)[1:]
    md = models.reshape(-1, n, models.shape[-1])
    return _reference(lambda b, t, x, v: _model_step(md[b if m_per else 0], powers, x, v),
                      x0, law, u_scale, noise, W, target, t_per, xs_mode, q_mode)


# ---------------------------------------------------------------- the device
def _law_args(law, B):
    """The law as the C ABI takes it: gains, x_ref, u_ref, law_per_instance, sat, du_band, du, u_prev, u_prev_per_instance."""
    per = 1 if (law.members == B and B > 1) else 0
    prev_per = 1 if (law.prev_members == B and B > 1) else 0
    band = law.du is not None
    return (_ptr(law.gains), _ptr(law.x_ref), _ptr(law.u_ref), per, law.sat, 1 if band else 0, law.du if band else 0.0,
            _ptr(law.u_prev) if band else None, prev_per if band else 0)


def _noise_args(noise):
    """noise_mode, sigma, sigma_per_instance, seed, member_base (and the array kept alive)."""
    if noise is None:
        return None, (0, None, 0, 0, 0)
    sigma = np.ascontiguousarray(noise.sigma.reshape(-1), dtype=np.float64)
    return sigma, (noise.mode, _ptr(sigma), 1 if noise.members is not None and noise.members > 1 else 0, noise.seed, noise.member_base)


def _extra_outputs(B, N, m, controls):
    us = np.empty((B, N, m), dtype=np.float64) if controls else None
    return us, np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)


def _result(xs, q, us, clipped, status):
    out = {}
    for name, a in (("xs", xs), ("q", q), ("us", us)):
        if a is not None:
            out[name] = a
    out["clipped"], out["status"] = clipped, status
    return out


def plant_feedback_batch(x0, law, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, noise=None, W=None, target=None,
                         keep="all", figure="none", controls=True):
    """N closed-loop steps of B plants under a stored law, in one launch: at every step the law reads the member's state (in
    registers), the member's plant advances under u_scale[b] * u_t over dts[t], and - with `noise`, a MeasurementNoise - the draw
    of (member, t + 1, component) is added to what is stored and carried on.

    x0 [B, n]; law a FeedbackLaw (shared or per member); op0, ops, dt_or_ts, kind, u_scale, W, target, keep, figure as
    plant_rollout_batch.  Returns a dict: "xs" and / or "q" as asked; with controls "us" [B, N, m], the commanded controls before
    u_scale; "clipped" [B] int32, the number of (t, k) at which a bound was active; "status" [B] int32, 0, or 3 when a state or
    control of the member was not finite."""
    kind = int(kind)
    x0, u_scale, W, target, t_per, xs_mode, q_mode = _prepare(x0, law, u_scale, noise, W, target, keep, figure,
                                                               kind != _lib.PLANT_PROCESS, "plant_feedback_batch")
    B, n = x0.shape
    N, m = law.N, law.m
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, N)
    xs, q = _outputs(B, N, n, xs_mode, q_mode)
    us, clipped, status = _extra_outputs(B, N, m, controls)
    sigma, nz = _noise_args(noise)
    L = _lib.lib()
    _lib.check(L.m4q_plant_feedback_batch(B, n, m, kind, N, _ptr(dts), _ptr(x0), *_law_args(law, B), _ptr(u_scale), _ptr(op0), _ptr(ops),
                                          per, *nz, _ptr(W), _ptr(target), t_per, xs_mode, _ptr(xs), q_mode, _ptr(q), _ptr(us),
                                          clipped.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
    return _result(xs, q, us, clipped, status)


def model_feedback_batch(x0, law, models, order, u_scale=None, noise=None, W=None, target=None, keep="all", figure="none",
                         controls=True):
    """plant_feedback_batch with the model x+ = A [x ; lift_u(u) (x) x] in the plant's place (models, order as model_rollout_batch):
    the law on the model it was designed on, or on an ensemble of fitted models."""
    x0, u_scale, W, target, t_per, xs_mode, q_mode = _prepare(x0, law, u_scale, noise, W, target, keep, figure, True,
                                                               "model_feedback_batch")
    B, n = x0.shape
    N, m = law.N, law.m
    models, order, m_per = _models(models, order, B, n, m)
    xs, q = _outputs(B, N, n, xs_mode, q_mode)
    us, clipped, status = _extra_outputs(B, N, m, controls)
    sigma, nz = _noise_args(noise)
    L = _lib.lib()
    _lib.check(L.m4q_model_feedback_batch(B, n, m, order, N, _ptr(x0), *_law_args(law, B), _ptr(u_scale), _ptr(models), m_per, *nz,
                                          _ptr(W), _ptr(target), t_per, xs_mode, _ptr(xs), q_mode, _ptr(q), _ptr(us),
                                          clipped.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
    return _result(xs, q, us, clipped, status)

"""Exit conditions the closed-loop kernel evaluates itself (include/m4q.h, m4q_session_set_exit).

The reference's mpc() takes any callable exit_condition(x_next, x, u) (mpc.py:289-291) and its tests use two of them: the gate
synthesis test's ((p1 - pf)^H Q (p1 - pf)).real < thr and abs(x_next[i]) > t.  Both are a thresholded quadratic form of one loop
state, which is what QuadraticExit describes.  The same object is such a callable (evaluated in NumPy, for the reference's mpc.py,
oracle.mpc and the host path) and, with a native plant, a condition the kernel checks for every ensemble member on its own."""
import numpy as np

from . import _lib

_STATES = {"prev": _lib.EXIT_PREV, "next": _lib.EXIT_NEXT}
_FIRES = {"below": _lib.EXIT_BELOW, "above": _lib.EXIT_ABOVE}


class QuadraticExit:
    """q(x) = Re((x - f)^H W (x - f)); fires when q(x) < thr (fires="below") or q(x) > thr (fires="above").

    x is the state an MPC step started from (state="prev": the reference's x, p1 of its synthesis test) or the state it produced
    (state="next": x_next, p2).  W [n, n] complex, shared by every member and not required to be Hermitian (the real part is
    taken); target f [n] shared or [B, n] per member; thr a scalar or [B] per member.  A member whose condition fires after MPC
    step k ends with exit code 1 and k valid steps: the attempted entry is dropped, as mpc.py:298-304 drops it.

    Called as exit_condition(x_next, x, u) it answers for one member (a per-member target or threshold needs `member`)."""

    def __init__(self, W, target, thr, state="prev", fires="below"):
        if state not in _STATES:
            raise ValueError("state must be 'prev' or 'next', got %r" % (state,))
        if fires not in _FIRES:
            raise ValueError("fires must be 'below' or 'above', got %r" % (fires,))
        W = np.array(W, dtype=np.complex128)
        if W.ndim != 2 or W.shape[0] != W.shape[1] or W.shape[0] < 1:
            raise ValueError("W must be a square matrix, got shape %s" % (W.shape,))
        n = W.shape[0]
        target = np.array(target, dtype=np.complex128)
        if target.ndim not in (1, 2) or target.shape[-1] != n or (target.ndim == 2 and target.shape[0] < 1):
            raise ValueError("target must have shape (%d,) or (B, %d), got %s" % (n, n, target.shape))
        thr = np.array(thr, dtype=np.float64)
        if thr.ndim > 1 or (thr.ndim == 1 and thr.shape[0] < 1):
            raise ValueError("thr must be a scalar or have shape (B,), got %s" % (thr.shape,))
        if target.ndim == 2 and thr.ndim == 1 and target.shape[0] != thr.shape[0]:
            raise ValueError("per-member target (%d rows) and threshold (%d entries) disagree on B" % (target.shape[0], thr.shape[0]))
        self.W, self.target, self.thr, self.state, self.fires = W, target, thr, state, fires

    @property
    def n(self):
        return self.W.shape[0]

    @property
    def members(self):
        """B if the target or the threshold is per member, else None."""
        if self.target.ndim == 2:
            return self.target.shape[0]
        return self.thr.shape[0] if self.thr.ndim == 1 else None

    @property
    def mode(self):
        """The M4Q_EXIT_* bits of m4q_session_set_exit."""
        return _STATES[self.state] | _FIRES[self.fires]

    def check(self, B, n):
        """ValueError unless the condition fits an ensemble of B members with n-dimensional states."""
        if self.n != n:
            raise ValueError("exit condition is %d-dimensional, the loop state %d-dimensional" % (self.n, n))
        if self.members is not None and self.members != B:
            raise ValueError("exit condition has per-member entries for %d members, the ensemble has %d" % (self.members, B))

    def block(self, lo, hi, B):
        """The condition of members [lo, hi) of an ensemble of B (per-member targets and thresholds sliced, shared ones kept)."""
        self.check(B, self.n)
        return QuadraticExit(self.W, self.target[lo:hi] if self.target.ndim == 2 else self.target,
                             self.thr[lo:hi] if self.thr.ndim == 1 else self.thr, self.state, self.fires)

    def value(self, x, member=None):
        """q(x) for one state x [n] (of member `member` where the target is per member)."""
        f = self._of(self.target, 2, member)
        d = np.asarray(x, dtype=np.complex128).reshape(-1) - f
        return float((d.conj() @ self.W @ d).real)

    def fired(self, x_next, x, member=None):
        q = self.value(x if self.state == "prev" else x_next, member)
        thr = float(self._of(self.thr, 1, member))
        return q < thr if self.fires == "below" else q > thr

    def __call__(self, x_next, x, u, member=None):
        return bool(self.fired(x_next, x, member))

    def _of(self, a, per_ndim, member):
        if a.ndim < per_ndim:
            return a
        if member is None:
            raise ValueError("this exit condition has per-member entries: pass member=")
        return a[member]

    def __repr__(self):
        return "QuadraticExit(n=%d, state=%r, fires=%r, members=%s)" % (self.n, self.state, self.fires, self.members)


def is_device_exit(cond):
    return isinstance(cond, QuadraticExit)


def require_device_exit(cond, where):
    """None or a QuadraticExit; TypeError for anything else (a plain callable cannot run on the device)."""
    if cond is not None and not isinstance(cond, QuadraticExit):
        raise TypeError("%s evaluates its exit condition on the device: pass a QuadraticExit (or None), not %r"
                        % (where, type(cond).__name__))
    return cond

"""The plant's own discrete-time Jacobians along trajectories, for whole ensembles in ONE launch (m4q_plant_linearize_batch): where
WrapModel.linearize_batch linearises a model - a truncated discretisation, or a fit - this linearises the held-control step of the
two unitary device plants itself, exactly.

The definition is here, in NumPy and SciPy.  Member b at point t is in state x = X[b, t] under the controls u = U[b|., t]; it sees
v_k = u_scale[b, k] u_k over the step length dts[t].  With X_e = -i dt (H0 + sum_k v_k H_k), E_k = -i dt H_k and
U, dU_k = grad._block_expm(X_e, E) (U = expm(X_e) and its Frechet derivatives, from one exponential of the (1 + m) d block matrix),
cols = 1 (Hamiltonian plant, n = d^2) or d^2 (process plant, n = d^4) and R = x.reshape(d, d, cols):
    A       = kron(kron(U, conj U), I_cols)                      [n, n]: it does not depend on the state
    B[:, k] = u_scale[b, k] vec(dU_k R U^H + U R dU_k^H)         the derivative with respect to the UNSCALED control u_k
    Delta   = -sum_k B[:, k] u_k, summed with k ascending from 0
The step is linear in the state, f(x, u) = A x, so A x + B u + Delta = f(x, u) to rounding, and the remainder of the expansion
around (x, u) is of second order in (dx, du).

Layouts are WrapModel.linearize_batch's: A [B, T, n, n], B [B, T, n, m], Delta [B, T, n], all complex, and go into
quad_program_batch unchanged.  Every shape is checked, and ValueError or TypeError raised, before the library is touched.  The
generator plant has no kernel (grad.py gives the reason): linearise its discretised model instead."""
import numpy as np

from . import _lib
from .grad import _block_expm
from .rollout import _plant_operators, _ptr, dts_of

OUTPUTS = ("A", "B", "Delta")


def _point(x, u, sc, H0, Hs, dt, kind):
    """(A, B, Delta) of one point: the module's definition, line by line."""
    m = u.shape[0]
    d = H0.shape[0]
    cols = 1 if kind == _lib.PLANT_HAMILTONIAN else d * d
    H = H0.astype(np.complex128)
    for k in range(m):
        H = H + (sc[k] * u[k]) * Hs[k]
    U, dUs = _block_expm(-1j * dt * H, [-1j * dt * Hs[k] for k in range(m)])
    A = np.kron(np.kron(U, U.conj()), np.identity(cols))
    R = x.reshape(d, d, cols)
    Bm = np.empty((x.shape[0], m), dtype=np.complex128)
    Delta = np.zeros(x.shape[0], dtype=np.complex128)
    for k in range(m):
        Bm[:, k] = sc[k] * (np.einsum('ac,cgx,eg->aex', dUs[k], R, U.conj()) + np.einsum('ac,cgx,eg->aex', U, R, dUs[k].conj())).reshape(-1)
        Delta = Delta - Bm[:, k] * u[k]
    return A, Bm, Delta


def _wanted(outputs):
    if isinstance(outputs, str) or not isinstance(outputs, (tuple, list)):
        raise TypeError('outputs must be a tuple of names out of "A", "B", "Delta", got %r' % (outputs,))
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError('outputs: %r is none of "A", "B", "Delta"' % (name,))
    if not outputs:
        raise ValueError("outputs is empty: nothing to return")
    return tuple(name in outputs for name in OUTPUTS)


def _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs):
    """Checks and lays out the arguments of the definition and of the device call alike."""
    want = _wanted(outputs)
    kind = int(kind)
    if kind == _lib.PLANT_GENERATOR:
        raise ValueError("the generator plant has no linearisation of its own on the device: discretise its generators "
                         "(discretize_homogeneous_batch) and linearise the model (WrapModel.linearize_batch)")
    X = np.asarray(X)
    if X.ndim != 3 or min(X.shape) < 1:
        raise ValueError("X must be [B, T, n] (the T linearisation points of B members), got shape %s" % (X.shape,))
    X = np.ascontiguousarray(X, dtype=np.complex128)
    B, T, n = X.shape
    U = np.asarray(U)
    if np.iscomplexobj(U):
        raise TypeError("U must be real")
    U = np.ascontiguousarray(U, dtype=np.float64)
    if U.ndim not in (2, 3) or U.shape[-2] != T or U.shape[-1] < 1 or (U.ndim == 3 and U.shape[0] not in (1, B)):
        raise ValueError("U must be [T, m] (shared) or [B|1, T, m] with B = %d, T = %d, got shape %s" % (B, T, U.shape))
    u_per = 1 if (U.ndim == 3 and U.shape[0] == B and B > 1) else 0
    m = U.shape[-1]
    if u_scale is not None:
        u_scale = np.ascontiguousarray(u_scale, dtype=np.float64)
        if u_scale.shape != (B, m):
            raise ValueError("u_scale must be [B, m] = (%d, %d), got %s" % (B, m, u_scale.shape))
    op0, ops, per = _plant_operators(op0, ops, kind, B, n, m)
    dts = dts_of(dt_or_ts, T)
    return X, U, u_per, u_scale, op0, ops, per, dts, kind, want


def plant_linearize_reference(X, U, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, outputs=OUTPUTS):
    """The definition of plant_linearize_batch (same arguments), on the host: SciPy's expm of the block matrix, point by point."""
    X, U, u_per, u_scale, op0, ops, per, dts, kind, want = _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs)
    B, T, n = X.shape
    m = U.shape[-1]
    k = op0.shape[-1]
    o0, ok, useq = op0.reshape(-1, k, k), ops.reshape(-1, m, k, k), U.reshape(-1, T, m)
    A = np.empty((B, T, n, n), dtype=np.complex128)
    Bm = np.empty((B, T, n, m), dtype=np.complex128)
    Delta = np.empty((B, T, n), dtype=np.complex128)
    for b in range(B):
        sc = np.ones(m) if u_scale is None else u_scale[b]
        for t in range(T):
            A[b, t], Bm[b, t], Delta[b, t] = _point(X[b, t], useq[b if u_per else 0, t], sc, o0[b if per else 0], ok[b if per else 0],
                                                    dts[t], kind)
    return tuple(a if w else None for a, w in zip((A, Bm, Delta), want))


def plant_linearize_batch(X, U, op0, ops, dt_or_ts, kind=_lib.PLANT_HAMILTONIAN, u_scale=None, outputs=OUTPUTS):
    """The exact Jacobians of the plant step at B T points in one launch.

    X [B, T, n] complex: the points; U [T, m] (shared) or [B|1, T, m] real: the controls as the caller passes them; op0, ops, kind as
    plant_rollout_batch (kind PLANT_HAMILTONIAN or PLANT_PROCESS: the generator plant is refused); dt_or_ts a scalar dt or a time
    grid of T + 1 points; u_scale [B, m]: member b sees u_scale[b] * u.  outputs: which of "A", "B", "Delta" to compute and copy back
    (A is 16 n^2 bytes per point and not always wanted).  Returns (A [B, T, n, n], B [B, T, n, m], Delta [B, T, n]), None for an
    output not asked for; what is returned does not depend on what else was asked for."""
    X, U, u_per, u_scale, op0, ops, per, dts, kind, want = _lin_common(X, U, op0, ops, dt_or_ts, kind, u_scale, outputs)
    B, T, n = X.shape
    m = U.shape[-1]
    A = np.empty((B, T, n, n), dtype=np.complex128) if want[0] else None
    Bm = np.empty((B, T, n, m), dtype=np.complex128) if want[1] else None
    Delta = np.empty((B, T, n), dtype=np.complex128) if want[2] else None
    L = _lib.lib()
    _lib.check(L.m4q_plant_linearize_batch(B, n, m, kind, T, _ptr(dts), _ptr(X), _ptr(U), u_per, _ptr(u_scale), _ptr(op0), _ptr(ops), per,
                                           _ptr(A), _ptr(Bm), _ptr(Delta)))
    return A, Bm, Delta

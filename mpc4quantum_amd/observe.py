"""Observed plants, defined once in NumPy (no torch; only observe_batch calls the device).

Two experiment classes of the reference close their loop on something other than the plant state: QCoupledExperiment (the plant
lives on the joint state of two qubits, the loop sees the two partial traces, experiment.py:238-306) and QExperiment32 (a three-level
plant, the loop sees its normalised qubit block, experiment.py:215-235).  An OBSERVED PLANT is that pair: a plant state z of
n_p = d_p^2 entries that evolves by the Hamiltonian plant's arithmetic (M4Q_PLANT_HAMILTONIAN), and the loop state x = observe(z) of
n = dim_x entries.  This module is the normative definition of observe (csrc/m4q_observe.h reproduces it, in this order of
operations); EnsembleSession.set_observed_plant / run_observed keep such a loop on the device.

OBSERVE_PARTIAL_TRACE (n_p = 16, n = 8, d_A = 2).  With r[a, b, a', b'] = z[(2a + b) 4 + 2a' + b']:
    x[2a + a']     = r[a, 0, a', 0] + r[a, 1, a', 1]        (trace over the second qubit)
    x[4 + 2b + b'] = r[0, b, 0, b'] + r[1, b, 1, b']        (trace over the first)
Two-term sums: the result does not depend on the order of summation, so the kernel, this module and both lifts agree bit for bit.

OBSERVE_QUBIT_BLOCK (n_p = 9, n = 4).  Bk = the leading 2 x 2 block of mat(z):
    F2  = |Bk00|^2 + |Bk01|^2 + |Bk10|^2 + |Bk11|^2         (|c|^2 = re re + im im, added in this order)
    det = Bk00 Bk11 - Bk01 Bk10,  |det| = sqrt(re re + im im)
    s   = sqrt(F2 + 2 |det|),     x = Bk / s                (real and imaginary part each divided by s)
s is the trace norm s1 + s2 of Bk - (s1 + s2)^2 = s1^2 + s2^2 + 2 s1 s2 = |Bk|_F^2 + 2 |det Bk| - which is what Qobj.unit() divides
by; the closed form needs no SVD on the device.  s = 0 gives NaN, as the reference's 0 / 0 does (the MPC kernel then ends that
member with exit code 3).  The kernel contracts re re + im im and the complex products into fused multiply-adds, so it agrees with
this module to a few roundings, not bit for bit; |det| squares the determinant, so blocks below 1e-77 in magnitude underflow."""
import numpy as np

from . import _lib

OBSERVE_PARTIAL_TRACE, OBSERVE_QUBIT_BLOCK = 1, 2    # M4Q_OBSERVE_* of include/m4q.h
_DIMS = {OBSERVE_PARTIAL_TRACE: (16, 8, 4), OBSERVE_QUBIT_BLOCK: (9, 4, 3)}      # kind -> (n_p, n, d_p)


def observe_dims(kind):
    """(n_p, n, d_p) of an observation kind: plant state, loop state, side of the plant's operators.  ValueError for any other."""
    try:
        return _DIMS[int(kind)]
    except (KeyError, TypeError, ValueError):
        raise ValueError("observe must be OBSERVE_PARTIAL_TRACE (1) or OBSERVE_QUBIT_BLOCK (2), got %r" % (kind,)) from None


def _plant_states(kind, z, where):
    n_p = observe_dims(kind)[0]
    z = np.asarray(z, dtype=np.complex128)
    if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] != n_p:
        raise ValueError("%s: z must have shape (B, %d) with B >= 1, got %s" % (where, n_p, z.shape))
    return np.ascontiguousarray(z)


def observe_reference(kind, z):
    """x [B, n] = observe(z) for plant states z [B, n_p]."""
    z = _plant_states(kind, z, "observe_reference")
    B = z.shape[0]
    if int(kind) == OBSERVE_PARTIAL_TRACE:
        r = z.reshape(B, 2, 2, 2, 2)
        xa = r[:, :, 0, :, 0] + r[:, :, 1, :, 1]
        xb = r[:, 0, :, 0, :] + r[:, 1, :, 1, :]
        return np.concatenate([xa.reshape(B, 4), xb.reshape(B, 4)], axis=1)
    bk = z.reshape(B, 3, 3)[:, :2, :2]
    f2 = np.zeros(B)
    for i in range(2):
        for j in range(2):
            f2 = f2 + (bk[:, i, j].real * bk[:, i, j].real + bk[:, i, j].imag * bk[:, i, j].imag)
    det = bk[:, 0, 0] * bk[:, 1, 1] - bk[:, 0, 1] * bk[:, 1, 0]
    s = np.sqrt(f2 + 2.0 * np.sqrt(det.real * det.real + det.imag * det.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = bk.real / s[:, None, None] + 1j * (bk.imag / s[:, None, None])
    return x.reshape(B, 4)


def check_observed_plant(kind, B, dim_x, dim_u, op0, ops, z0, where):
    """The arrays m4q_session_set_observed_plant reads, as (op0 [B|1, d_p, d_p], ops [B|1, m, d_p, d_p], per_instance, z0 [B, n_p]):
    ValueError for a kind that does not fit dim_x or any other shape.  The C side takes the sizes from the session, not from the
    arrays: anything else would be read past its end."""
    n_p, n, d = observe_dims(kind)
    B, m = int(B), int(dim_u)
    if int(dim_x) != n:
        raise ValueError("%s: observe=%d gives loop states of %d entries, the session has dim_x=%d" % (where, int(kind), n, dim_x))
    op0 = np.asarray(op0, dtype=np.complex128)
    ops = np.asarray(ops, dtype=np.complex128)
    if op0.ndim == 2:
        op0 = op0[None]
    if ops.ndim == 3:
        ops = ops[None]
    if op0.ndim != 3 or op0.shape[1:] != (d, d) or op0.shape[0] not in (1, B):
        raise ValueError("%s: op0 must have shape (%d, %d), (1, %d, %d) or (%d, %d, %d), got %s" % (where, d, d, d, d, B, d, d, op0.shape))
    if ops.ndim != 4 or ops.shape[1:] != (m, d, d) or ops.shape[0] not in (1, B):
        raise ValueError("%s: ops must have shape (%d, %d, %d), (1, %d, %d, %d) or (%d, %d, %d, %d), got %s"
                         % (where, m, d, d, m, d, d, B, m, d, d, ops.shape))
    per = op0.shape[0] > 1 or ops.shape[0] > 1
    if per:                                       # the kernel reads both with the member's stride
        op0 = np.broadcast_to(op0, (B, d, d))
        ops = np.broadcast_to(ops, (B, m, d, d))
    z0 = np.asarray(z0, dtype=np.complex128)
    if z0.shape != (B, n_p):
        raise ValueError("%s: the plant states must have shape (%d, %d), got %s" % (where, B, n_p, z0.shape))
    return np.ascontiguousarray(op0), np.ascontiguousarray(ops), int(per), np.ascontiguousarray(z0)


def observed_plant_step_reference(kind, z, u, op0, ops, dt):
    """(z_next [B, n_p], x_next [B, n]): one held-control step of the Hamiltonian plant, rho+ = U rho U^H with
    U = expm(-i dt (H0 + sum_k u_k H_k)) (SciPy's expm, member by member), followed by observe.  z [B, n_p], u [B, m],
    op0 [B|1, d_p, d_p] (or [d_p, d_p]), ops [B|1, m, d_p, d_p] (or [m, d_p, d_p])."""
    from scipy.linalg import expm
    z = _plant_states(kind, z, "observed_plant_step_reference")
    B = z.shape[0]
    u = np.asarray(u, dtype=np.float64)
    if u.ndim != 2 or u.shape[0] != B:
        raise ValueError("observed_plant_step_reference: u must have shape (%d, m), got %s" % (B, u.shape))
    op0, ops, per, z = check_observed_plant(kind, B, observe_dims(kind)[1], u.shape[1], op0, ops, z, "observed_plant_step_reference")
    d = observe_dims(kind)[2]
    zn = np.empty_like(z)
    for b in range(B):
        H = op0[b if per else 0] + np.tensordot(u[b], ops[b if per else 0], axes=1)
        U = expm(-1j * float(dt) * H)
        zn[b] = (U @ z[b].reshape(d, d) @ U.conj().T).reshape(-1)
    return zn, observe_reference(kind, zn)


def observe_batch(kind, z):
    """observe_reference on the device (m4q_observe_batch, the kernel the closed loop calls): z [B, n_p] -> x [B, n]."""
    z = _plant_states(kind, z, "observe_batch")
    out = np.empty((z.shape[0], observe_dims(kind)[1]), dtype=np.complex128)
    _lib.check(_lib.lib().m4q_observe_batch(z.shape[0], int(kind), _lib.cbuf(z)[1], out.ctypes.data_as(_lib._dp)))
    return out

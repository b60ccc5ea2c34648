"""Measurement noise of the closed loop, defined once in NumPy (no torch, no device call).

The reference's QExperiment.set_sigma adds complex Gaussian noise of standard deviation sigma to what `simulate` returns
(experiment.py:188-212), and mpc.py:259-260 stores that column as xs[step + 1]: every later linearisation, QP, plant step and exit
condition sees it.  This module is the normative definition of the noise the kernel adds at that point (csrc/m4q_noise.h
reproduces it): a counter-based generator, so a draw depends on the seed, the GLOBAL ensemble member, the column of xs it lands in
and the component of the loop state - and on nothing else (not the launch, the resident row, the work item or the rank).

Bits: Philox4x32-10 (Salmon et al., Random123).  key = (seed & 0xffffffff, seed >> 32); counter = (member & 0xffffffff,
member >> 32, state_index, component); state_index = step + 1 (never 0: x0 is not measured), component = row-major index 0..n-1.
Unit complex normal from the four output words w0..w3:
    u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53   in (0, 1]      u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53   in [0, 1)
    z = sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2),    |z| <= sqrt(106 ln 2) ~ 8.57
Kinds: "iid" adds sigma z to every component (the reference's noise as written; it does not keep a density matrix Hermitian);
"hermitian" adds E = sigma ((Z + Z^H) / 2 - (Re tr Z / d) I) with Z[a][b] = z of component a d + b: Hermitian and traceless, so a
Hermitian state of given trace stays one (the extension the reference's TODO at experiment.py:179-181 asks for)."""
import math

import numpy as np

NOISE_IID, NOISE_HERMITIAN = 1, 2                    # M4Q_NOISE_* of include/m4q.h
_KINDS = {"iid": NOISE_IID, "hermitian": NOISE_HERMITIAN}
Z_MAX = math.sqrt(106.0 * math.log(2.0))             # |z| of u1 = 2^-53

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10.  counter [..., 4], key [..., 2] (broadcast against each other), 32-bit words held in uint64; returns the
    four output words [..., 4] as uint64 below 2^32."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1)


def uniforms(words):
    """(u1 in (0, 1], u2 in [0, 1)) from output words [..., 4]: 53-bit integers scaled by 2^-53, every value exact in fp64."""
    w = np.asarray(words, dtype=np.uint64)
    hi1, lo1 = (w[..., 0] >> np.uint64(5)).astype(np.float64), (w[..., 1] >> np.uint64(6)).astype(np.float64)
    hi2, lo2 = (w[..., 2] >> np.uint64(5)).astype(np.float64), (w[..., 3] >> np.uint64(6)).astype(np.float64)
    return (hi1 * 67108864.0 + lo1 + 1.0) * 2.0 ** -53, (hi2 * 67108864.0 + lo2) * 2.0 ** -53


def box_muller(u1, u2):
    r = np.sqrt(-2.0 * np.log(u1))
    return r * (np.cos(2.0 * np.pi * u2) + 1j * np.sin(2.0 * np.pi * u2))


def unit_normal(seed, members, state_index, n):
    """z [len(members), n]: the unit complex normal of every (member, state_index, component)."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    state_index, n = int(state_index), int(n)
    if not 1 <= state_index < 1 << 32:
        raise ValueError("state_index must be in [1, 2^32): x0 is not measured, got %d" % state_index)
    if n < 1:
        raise ValueError("n must be positive, got %d" % n)
    mem = [int(v) for v in np.asarray(members).reshape(-1).tolist()]
    if any(not 0 <= v < 1 << 64 for v in mem):
        raise ValueError("members must be in [0, 2^64)")
    mem = np.array(mem, dtype=np.uint64).reshape(-1, 1)
    counter = np.empty((mem.shape[0], n, 4), dtype=np.uint64)
    counter[..., 0] = mem & _LO
    counter[..., 1] = mem >> _S32
    counter[..., 2] = np.uint64(state_index)
    counter[..., 3] = np.arange(n, dtype=np.uint64)[None, :]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return box_muller(*uniforms(philox4x32(counter, key)))


def hermitian_part(z, d):
    """(Z + Z^H) / 2 - (Re tr Z / d) I for z [..., d d] (row-major Z): Hermitian exactly, traceless to rounding."""
    Z = np.asarray(z).reshape(z.shape[:-1] + (d, d))
    H = (Z + np.conj(np.swapaxes(Z, -1, -2))) * 0.5
    t = np.zeros(Z.shape[:-2])
    for c in range(d):                               # (summed in index order, as the kernel sums it)
        t = t + Z[..., c, c].real
    H = H - (t / d)[..., None, None] * np.eye(d)
    return H.reshape(z.shape)


def square_dim(n):
    d = int(math.isqrt(int(n)))
    return d if d * d == n else 0


class MeasurementNoise:
    """Measurement noise the closed-loop kernel draws itself: xs[member, :, step + 1] += sample(member, step + 1, n) on every
    measured step.

    sigma: a scalar or [B] per member, >= 0.  seed: integer in [0, 2^64).  kind: "iid" (sigma z on every component: the
    reference's set_sigma; runs the complex path) or "hermitian" (Hermitian and traceless: keeps every arithmetic path; needs a
    density-matrix state, n = d d).  member_base: the global index of this ensemble's member 0."""

    def __init__(self, sigma, seed, kind="iid", member_base=0):
        if kind not in _KINDS:
            raise ValueError("kind must be 'iid' or 'hermitian', got %r" % (kind,))
        sigma = np.array(sigma, dtype=np.float64)
        if sigma.ndim > 1 or (sigma.ndim == 1 and sigma.shape[0] < 1):
            raise ValueError("sigma must be a scalar or have shape (B,), got %s" % (sigma.shape,))
        if not np.all(np.isfinite(sigma)) or np.any(sigma < 0):
            raise ValueError("sigma must be finite and >= 0")
        seed, member_base = int(seed), int(member_base)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
        if not 0 <= member_base < 1 << 64:
            raise ValueError("member_base must be an integer in [0, 2^64), got %r" % (member_base,))
        self.sigma, self.seed, self.kind, self.member_base = sigma, seed, kind, member_base

    @property
    def mode(self):
        """The M4Q_NOISE_* value of m4q_session_set_noise."""
        return _KINDS[self.kind]

    @property
    def members(self):
        """B if sigma is per member, else None."""
        return self.sigma.shape[0] if self.sigma.ndim == 1 else None

    def check(self, B, n):
        """ValueError unless the noise fits an ensemble of B members with n-dimensional states."""
        if self.members is not None and self.members != B:
            raise ValueError("noise has a sigma for %d members, the ensemble has %d" % (self.members, B))
        if self.kind == "hermitian" and not square_dim(n):
            raise ValueError("hermitian noise needs a density-matrix state (n = d d), got n = %d" % n)
        if self.member_base + B > 1 << 64:
            raise ValueError("member_base + B exceeds 2^64")

    def block(self, lo, hi, B):
        """The noise of members [lo, hi) of an ensemble of B: sigma sliced, member_base advanced - the same draws per member."""
        if self.members is not None and self.members != B:
            raise ValueError("noise has a sigma for %d members, the ensemble has %d" % (self.members, B))
        return MeasurementNoise(self.sigma[lo:hi] if self.sigma.ndim == 1 else self.sigma, self.seed, self.kind,
                                self.member_base + lo)

    def _global(self, members):
        return [self.member_base + int(v) for v in np.asarray(members).reshape(-1).tolist()]

    def unit(self, members, state_index, n):
        """z [len(members), n] for the LOCAL member indices given (member_base is added)."""
        return unit_normal(self.seed, self._global(members), state_index, n)

    def sample(self, members, state_index, n):
        """The noise added to xs[members, :, state_index], [len(members), n] complex, for either kind."""
        members = np.asarray(members).reshape(-1)
        z = self.unit(members, state_index, n)
        if self.kind == "hermitian":
            d = square_dim(n)
            if not d:
                raise ValueError("hermitian noise needs a density-matrix state (n = d d), got n = %d" % n)
            z = hermitian_part(z, d)
        if self.sigma.ndim == 1:
            if members.size and (members.min() < 0 or members.max() >= self.sigma.shape[0]):
                raise ValueError("member index outside the %d entries of sigma" % self.sigma.shape[0])
            return self.sigma[members][:, None] * z
        return float(self.sigma) * z

    def __repr__(self):
        return "MeasurementNoise(kind=%r, seed=%d, member_base=%d, members=%s)" % (self.kind, self.seed, self.member_base,
                                                                                   self.members)


def require_noise(noise, where):
    """None or a MeasurementNoise; TypeError for anything else."""
    if noise is not None and not isinstance(noise, MeasurementNoise):
        raise TypeError("%s takes a MeasurementNoise (or None), not %r" % (where, type(noise).__name__))
    return noise


def check_batch_noise(noise, B, n, plant_kind, where):
    """TypeError / ValueError unless `noise` is None or fits an ensemble of B members, n-dimensional states and the plant kind
    (M4Q_PLANT_* value); raised before any device call."""
    require_noise(noise, where)
    if noise is None:
        return
    noise.check(B, n)
    if plant_kind == 0:
        raise ValueError("%s: measurement noise needs a device plant (with PLANT_NONE the host supplies the states)" % where)
    if plant_kind == 3 and noise.kind == "hermitian":
        raise ValueError("%s: hermitian noise needs a density-matrix loop state; a process plant's is a process vector "
                         "(use kind='iid')" % where)

"""Measurement noise on the host (no device): the counter-based generator of mpc4quantum_amd/noise.py against known answers, the
distribution of its draws, the Hermitian kind, independence from grouping, the refusals the entry points raise before any device
call, and the stepwise path of mpc() against a stub session.

The statistical bounds are six standard errors derived from N; the runs are deterministic (fixed seeds), so a bound that fails
is a bug and not bad luck."""
import math
import os
import sys

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs, noise as nz
from mpc4quantum_amd.mpc import mpc_batch, open_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. bits
def _words(hexes):
    return [int(h, 16) for h in hexes.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    out = nz.philox4x32(np.array(_words(counter), dtype=np.uint64), np.array(_words(key), dtype=np.uint64))
    assert [int(v) for v in out] == _words(want)


def test_philox_is_vectorised_consistently():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 1 << 32, size=(7, 5, 4), dtype=np.uint64)
    k = rng.integers(0, 1 << 32, size=(2,), dtype=np.uint64)
    out = nz.philox4x32(c, k)
    for i in (0, 3, 6):
        for j in (0, 4):
            assert np.array_equal(out[i, j], nz.philox4x32(c[i, j], k))


def test_counter_layout():
    """key = (seed lo, seed hi); counter = (member lo, member hi, state_index, component)."""
    seed, member, sidx, n = 0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e, 6
    z = nz.unit_normal(seed, [member], sidx, n)[0]
    for comp in range(n):
        w = nz.philox4x32(np.array([0x243f6a88, 0x85a308d3, 0x13198a2e, comp], dtype=np.uint64),
                          np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
        assert z[comp] == nz.box_muller(*nz.uniforms(w))
    with pytest.raises(ValueError):
        nz.unit_normal(seed, [0], 0, n)                           # x0 is not measured
    with pytest.raises(ValueError):
        nz.unit_normal(1 << 64, [0], 1, n)


# ---------------------------------------------------------------- 2. uniforms
def test_uniforms_exact_and_in_range_at_the_extremes():
    zero = np.zeros(4, dtype=np.uint64)
    ones = np.full(4, 0xFFFFFFFF, dtype=np.uint64)
    u1, u2 = nz.uniforms(zero)
    assert u1 == 2.0 ** -53 and u2 == 0.0
    u1, u2 = nz.uniforms(ones)
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -53
    # every value is k 2^-53 with k a 53-bit integer: exact
    rng = np.random.default_rng(1)
    w = rng.integers(0, 1 << 32, size=(1000, 4), dtype=np.uint64)
    u1, u2 = nz.uniforms(w)
    k1 = (w[:, 0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[:, 1] >> np.uint64(6)) + np.uint64(1)
    k2 = (w[:, 2] >> np.uint64(5)) * np.uint64(1 << 26) + (w[:, 3] >> np.uint64(6))
    assert np.array_equal((u1 * 2.0 ** 53).astype(np.uint64), k1) and np.array_equal((u2 * 2.0 ** 53).astype(np.uint64), k2)
    assert np.all(u1 > 0) and np.all(u1 <= 1) and np.all(u2 >= 0) and np.all(u2 < 1)
    # |z| at the smallest u1
    assert abs(abs(nz.box_muller(np.float64(2.0 ** -53), np.float64(0.25))) - nz.Z_MAX) < 1e-14 and 8.5 < nz.Z_MAX < 8.6


# ---------------------------------------------------------------- 3. distribution of the replica
def _corr(a, b):
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def test_distribution_of_unit_draws():
    members, n, sidxs = 4096, 16, 16                  # N = 2^20 draws
    noise = m4q.MeasurementNoise(1.0, seed=20240917)
    z = np.stack([noise.unit(np.arange(members), s + 1, n) for s in range(sidxs)], axis=0)      # [state_index, member, component]
    N = z.size
    assert N >= 1 << 20
    se = 1.0 / math.sqrt(N)
    re, im = z.real.ravel(), z.imag.ravel()
    print("N=%d mean re %.3e im %.3e var re %.6f im %.6f corr(re, im) %.3e max|z| %.3f"
          % (N, re.mean(), im.mean(), re.var(), im.var(), _corr(re, im), np.abs(z).max()))
    assert abs(re.mean()) <= 6 * se and abs(im.mean()) <= 6 * se
    assert abs(re.var() - 1.0) <= 6 * math.sqrt(2.0 / N) and abs(im.var() - 1.0) <= 6 * math.sqrt(2.0 / N)
    assert abs(_corr(re, im)) <= 6 * se
    assert np.abs(z).max() <= nz.Z_MAX
    # neighbours along each counter word (pairs: N less one slice, the bound from the number of pairs)
    for axis, name in ((0, "state index"), (1, "member"), (2, "component")):
        a = np.take(z, range(0, z.shape[axis] - 1), axis=axis)
        b = np.take(z, range(1, z.shape[axis]), axis=axis)
        for pa, pb, tag in ((a.real, b.real, "re-re"), (a.imag, b.imag, "im-im"), (a.real, b.imag, "re-im")):
            c = _corr(pa.ravel(), pb.ravel())
            print("neighbouring %s %s: %.3e" % (name, tag, c))
            assert abs(c) <= 6 / math.sqrt(pa.size), (name, tag, c)


# ---------------------------------------------------------------- 4. the Hermitian kind
@pytest.mark.parametrize("d", [2, 3, 4])
def test_hermitian_kind(d):
    n, B, sigma = d * d, 1 << 16, 0.37
    noise = m4q.MeasurementNoise(sigma, seed=99, kind="hermitian")
    E = noise.sample(np.arange(B), 3, n).reshape(B, d, d)
    assert np.array_equal(E, np.conj(np.swapaxes(E, 1, 2)))                        # exactly Hermitian
    tr = np.trace(E, axis1=1, axis2=2)
    ulp = np.spacing(sigma * nz.Z_MAX)
    assert np.abs(tr).max() <= d * ulp, (np.abs(tr).max(), d * ulp)
    diag = np.stack([E[:, a, a].real for a in range(d)], axis=1).ravel()
    off = np.stack([E[:, a, b] for a in range(d) for b in range(d) if a < b], axis=1).ravel()
    vd, vo = sigma ** 2 * (1.0 - 1.0 / d), sigma ** 2 / 2.0
    # standard errors.  Off-diagonal parts are independent normals: the variance estimate of N of them has standard error
    # var sqrt(2 / N).  The d diagonal entries of one member are d independent N(0, sigma^2) projected onto the sum-zero subspace:
    # their squares add up to sigma^2 chi^2_{d-1} (variance 2 (d - 1) sigma^4), so the pooled estimate over B members and d entries
    # has variance 2 (d - 1) sigma^4 / (B d^2) = vd^2 * 2 / (B (d - 1)).
    assert abs(np.mean(diag ** 2) - vd) <= 6 * vd * math.sqrt(2.0 / (B * (d - 1))), (np.mean(diag ** 2), vd)
    assert abs(E[:, 0, 0].real.mean()) <= 6 * math.sqrt(vd / B)
    for part in (off.real, off.imag):
        assert abs(part.var() - vo) <= 6 * vo * math.sqrt(2.0 / part.size), (part.var(), vo)
        assert abs(part.mean()) <= 6 * math.sqrt(vo / part.size)
    # built from the same draws z as the iid kind
    z = m4q.MeasurementNoise(1.0, seed=99).unit(np.arange(8), 3, n)
    assert np.array_equal(E[:8].reshape(8, n), sigma * nz.hermitian_part(z, d))


def test_iid_kind_is_sigma_z():
    noise = m4q.MeasurementNoise([0.0, 0.5, 2.0], seed=5)
    z = noise.unit([0, 1, 2], 7, 9)
    assert np.array_equal(noise.sample([0, 1, 2], 7, 9), np.array([0.0, 0.5, 2.0])[:, None] * z)
    assert np.array_equal(noise.sample([2], 7, 9)[0], 2.0 * z[2])


# ---------------------------------------------------------------- 5. independence from grouping
@pytest.mark.parametrize("kind", ["iid", "hermitian"])
def test_independent_of_grouping(kind):
    noise = m4q.MeasurementNoise(0.1, seed=1234567890123, kind=kind)
    full = noise.sample(np.arange(100), 4, 9)
    assert np.array_equal(noise.sample([5, 6, 7], 4, 9), full[5:8])
    k = (1 << 32) - 2                                                                  # straddles the low counter word
    based = m4q.MeasurementNoise(0.1, seed=1234567890123, kind=kind, member_base=k)
    assert np.array_equal(based.sample(np.arange(5), 4, 9), noise.sample(np.arange(k, k + 5), 4, 9))
    assert not np.array_equal(based.sample([1], 4, 9), based.sample([2], 4, 9))
    # block(): what rank r of a sharded run passes
    per = m4q.MeasurementNoise(np.linspace(0.0, 1.0, 11), seed=3, kind=kind, member_base=40)
    blk = per.block(6, 11, 11)
    assert blk.member_base == 46 and np.array_equal(blk.sigma, per.sigma[6:]) and blk.members == 5
    assert np.array_equal(blk.sample(np.arange(5), 2, 4), per.sample(np.arange(6, 11), 2, 4))
    assert noise.block(6, 11, 11).members is None and noise.block(6, 11, 11).member_base == 6


# ---------------------------------------------------------------- 6. refusals, before any device call
def test_object_refusals():
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(0.1, 0, kind="white")
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(-0.1, 0)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise([0.1, -1e-9], 0)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(float("nan"), 0)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(np.zeros((2, 2)), 0)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(0.1, -1)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(0.1, 0, member_base=1 << 64)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(np.zeros(3), 0).check(4, 9)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(0.1, 0, kind="hermitian").check(4, 8)
    with pytest.raises(ValueError):
        m4q.MeasurementNoise(0.1, 0, kind="hermitian").sample([0], 1, 8)
    assert m4q.MeasurementNoise(0.1, 0).mode == _lib.NOISE_IID == nz.NOISE_IID
    assert m4q.MeasurementNoise(0.1, 0, kind="hermitian").mode == _lib.NOISE_HERMITIAN == nz.NOISE_HERMITIAN


def _fail_session(*a, **k):
    raise AssertionError("a device session was opened")


def test_batch_entry_points_reject_before_the_device(monkeypatch):
    monkeypatch.setattr(sys.modules["mpc4quantum_amd.mpc"], "EnsembleSession", _fail_session)
    p = configs.build(2, batch=3, horizon=4, n_steps=2)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    args = (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
            p["R"], p["Qf"], p["sat"], p["du"])
    from mpc4quantum_amd.distributed import mpc_batch_sharded
    for entry in (mpc_batch, open_session, mpc_batch_sharded):          # (sharded, transport=None: raised before RCCL is touched)
        with pytest.raises(TypeError):
            entry(*args, noise=0.1)
        with pytest.raises(TypeError):
            entry(*args, noise=lambda *a: 0.0)
        with pytest.raises(ValueError):
            entry(*args, noise=m4q.MeasurementNoise(np.full(5, 0.1), 1))                          # sigma of the wrong length
        with pytest.raises(ValueError):
            entry(*args, plant_kind=_lib.PLANT_NONE, noise=m4q.MeasurementNoise(0.1, 1))
        with pytest.raises(ValueError):
            entry(*args, plant_kind=_lib.PLANT_NONE, noise=m4q.MeasurementNoise(0.1, 1, kind="hermitian"))
    # hermitian on a process plant; hermitian with a state that is no density matrix
    s = configs.synthesis(batch=2, horizon=4, n_steps=2)
    sclock = m4q.StepClock(s["dt"], s["horizon"], s["n_steps"])
    sargs = (s["x0"], s["models"], s["dim_u"], s["order"], s["X_targ"], s["U_targ"], sclock, s["plant_op0"], s["plant_ops"], s["Q"],
             s["R"], s["Qf"], s["sat"], s["du"])
    for entry in (mpc_batch, open_session, mpc_batch_sharded):
        with pytest.raises(ValueError):
            entry(*sargs, plant_kind=_lib.PLANT_PROCESS, noise=m4q.MeasurementNoise(0.1, 1, kind="hermitian"))
    x8 = np.zeros((3, 8), dtype=complex)
    with pytest.raises(ValueError):
        mpc_batch(x8, *args[1:], noise=m4q.MeasurementNoise(0.1, 1, kind="hermitian"))


def test_experiment_set_noise_refusals():
    H = [np.diag([1.0, -1.0]).astype(complex), np.array([[0, 1], [1, 0]], dtype=complex)]
    for exp in (m4q.QExperiment(H[0], H[1:]), m4q.QSynthesis(H[0], H[1:])):
        assert exp.device_noise is None
        with pytest.raises(TypeError):
            exp.set_noise(0.1)
        noise = m4q.MeasurementNoise(0.1, 1)
        exp.set_noise(noise)
        assert exp.device_noise is noise
        exp.set_noise(None)
        assert exp.device_noise is None


def test_capi_set_noise_null_session():
    L = _lib.lib()
    one = np.full(1, 0.1)
    assert L.m4q_session_set_noise(None, _lib.NOISE_IID, one.ctypes.data_as(_lib._dp), 0, 1, 0) == _lib.E_BADARG
    assert b"null session" in L.m4q_last_error()
    out = np.zeros(8)
    # argument refusals of the sampling entry point come before it looks for a device
    assert L.m4q_noise_sample_batch(1, 4, 3, one.ctypes.data_as(_lib._dp), 0, 1, 0, 1, out.ctypes.data_as(_lib._dp)) == _lib.E_BADARG
    assert L.m4q_noise_sample_batch(1, 4, _lib.NOISE_IID, one.ctypes.data_as(_lib._dp), 0, 1, 0, 0,
                                    out.ctypes.data_as(_lib._dp)) == _lib.E_BADARG                # state_index 0
    neg = np.full(1, -0.1)
    assert L.m4q_noise_sample_batch(1, 4, _lib.NOISE_IID, neg.ctypes.data_as(_lib._dp), 0, 1, 0, 1,
                                    out.ctypes.data_as(_lib._dp)) == _lib.E_BADARG
    assert L.m4q_noise_sample_batch(1, 8, _lib.NOISE_HERMITIAN, one.ctypes.data_as(_lib._dp), 0, 1, 0, 1,
                                    np.zeros(16).ctypes.data_as(_lib._dp)) == _lib.E_BADARG       # n = 8 is not d d
    assert L.m4q_noise_sample_batch(1, 5, _lib.NOISE_IID, one.ctypes.data_as(_lib._dp), 0, 1, 0, 1,
                                    np.zeros(10).ctypes.data_as(_lib._dp)) == _lib.E_UNSUPPORTED  # no kernel with dim_x = 5


# ---------------------------------------------------------------- 7. mpc(): the stepwise path, against a stub session
class _StubSession:
    """Stands for EnsembleSession on the host path of mpc(): every step 'solves' to a fixed control and records the states the
    loop hands back (put_state).  No device, no library."""
    instances = []

    def __init__(self, B, n, m, order, T, ns, *a, **kw):
        self.n, self.m, self.ns = n, m, ns
        self.plant_kind = kw.get("plant_kind")
        self.force_complex = kw.get("force_complex")
        self.states = {}
        self.noise_set = None
        _StubSession.instances.append(self)

    def load_problem(self, *a, **k):
        pass

    def set_noise(self, noise):
        self.noise_set = noise

    def run(self, a, b):
        pass

    def sync(self):
        pass

    def download(self, field, shape):
        if field == _lib.F_CODES:
            return np.zeros(shape, dtype=np.int32)
        return np.full(shape, 0.25)

    def put_state(self, step, x):
        self.states[step] = np.array(x).reshape(-1)

    def close(self):
        pass


class _Model:
    def __init__(self, A):
        self.A = A

    def get_discrete(self):
        n = self.A.shape[0]
        return self.A[:, :n], self.A[:, n:]

    def predict(self, lx, lux):
        Ax, Au = self.get_discrete()
        return Ax @ lx + Au @ lux


class _ForeignPlant(m4q.Experiment):
    """A host plant that is none of this package's: x+ = 0.9 x + 0.01 u, deterministic."""

    def f(self, t, x, u):
        return x

    def simulate(self, x0, ts, us):
        x = np.asarray(x0, dtype=complex).reshape(-1)
        cols = [x]
        for i in range(len(ts) - 1):
            x = 0.9 * x + 0.01 * float(np.real(us(ts[i]))[0])
            cols.append(x)
        return np.stack(cols, axis=1)


@pytest.mark.parametrize("mf", [1, 2])
@pytest.mark.parametrize("kind", ["iid", "hermitian"])
def test_mpc_stepwise_adds_the_draws_of_member_base(monkeypatch, mf, kind):
    monkeypatch.setattr(sys.modules["mpc4quantum_amd.mpc"], "EnsembleSession", _StubSession)
    _StubSession.instances.clear()
    p = configs.build(1, horizon=4, n_steps=6)
    n, m = p["dim_x"], p["dim_u"]
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    clock.measure_freq = mf
    plant = _ForeignPlant()
    noise = m4q.MeasurementNoise(1e-2, seed=77, kind=kind, member_base=12345)
    plant.device_noise = noise
    model = _Model(p["models"][0])
    (xs, us), _, code = m4q.mpc(p["x0"][0], m, 1, p["X_targ"], p["U_targ"], clock, plant, model, p["Q"], p["R"], p["Qf"], p["sat"],
                                p["du"], progress_bar=False)
    assert code == 0 and xs.shape == (n, 7) and us.shape == (m, 6)
    sess = _StubSession.instances[-1]
    assert sess.plant_kind == _lib.PLANT_NONE and sess.noise_set is None          # the host supplies the states, noise included
    assert bool(sess.force_complex) == (kind == "iid")                           # states that are not Hermitian: the complex path
    ref = m4q.MeasurementNoise(1e-2, seed=77, kind=kind)
    for step in range(6):
        if (step + 1) % mf == 0:
            clean = xs[:, step + 1 - mf]
            for _ in range(mf):
                clean = 0.9 * clean + 0.01 * 0.25
            want = clean + ref.sample([12345], step + 1, n)[0]
            assert np.array_equal(xs[:, step + 1], want), step
        assert np.array_equal(sess.states[step + 1], xs[:, step + 1])                # what the next QP starts from
    # no noise object: the same loop is noise-free
    plant.device_noise = None
    (xs0, _), _, _ = m4q.mpc(p["x0"][0], m, 1, p["X_targ"], p["U_targ"], clock, plant, model, p["Q"], p["R"], p["Qf"], p["sat"],
                             p["du"], progress_bar=False)
    assert np.allclose(xs0[:, mf], 0.9 ** mf * xs0[:, 0] + sum(0.9 ** i for i in range(mf)) * 0.0025, rtol=0, atol=1e-15)
    assert not np.array_equal(xs0[:, mf], xs[:, mf])


def test_mpc_refuses_both_noises_and_a_wrong_object(monkeypatch):
    monkeypatch.setattr(sys.modules["mpc4quantum_amd.mpc"], "EnsembleSession", _fail_session)
    p = configs.build(1, horizon=4, n_steps=3)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    H = [np.diag([1.0, -1.0]).astype(complex), np.array([[0, 1], [1, 0]], dtype=complex)]
    exp = m4q.QExperiment(H[0], H[1:])
    exp.set_noise(m4q.MeasurementNoise(1e-3, 1))
    exp.set_sigma(1e-3)
    model = _Model(p["models"][0])
    args = (p["x0"][0], p["dim_u"], 1, p["X_targ"], p["U_targ"], clock, exp, model, p["Q"], p["R"], p["Qf"], p["sat"], p["du"])
    with pytest.raises(ValueError):
        m4q.mpc(*args, progress_bar=False)
    exp.set_sigma(0)
    exp.device_noise = 0.1
    with pytest.raises(TypeError):
        m4q.mpc(*args, progress_bar=False)
    exp.set_noise(m4q.MeasurementNoise([1e-3, 1e-3], 1))                          # a [2] sigma for the one member of mpc()
    with pytest.raises(ValueError):
        m4q.mpc(*args, progress_bar=False)


def test_set_sigma_alone_still_takes_the_host_path():
    from mpc4quantum_amd.mpc import _native_plant, _runs_fused
    H = [np.diag([1.0, -1.0]).astype(complex), np.array([[0, 1], [1, 0]], dtype=complex)]
    exp = m4q.QExperiment(H[0], H[1:])
    exp.set_noise(m4q.MeasurementNoise(1e-3, 1))
    assert _native_plant(exp) and _runs_fused(exp, None, False)                   # device noise keeps the loop fused
    assert not _runs_fused(exp, lambda xn, x, u: False, False)
    exp.set_noise(None)
    exp.set_sigma(1e-3)
    assert not _native_plant(exp) and not _runs_fused(exp, None, False)


# ---------------------------------------------------------------- the device header, compiled for the host
_HIP_STUB = r'''
#pragma once
#include <cmath>
#define __device__
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline void sincospi(double x, double* s, double* c) { *s = std::sin(M_PI * x); *c = std::cos(M_PI * x); }
'''
_HARNESS = r'''
#include <cstdio>
#include <cstdlib>
namespace m4q { struct cplx { double re, im; }; }
#include "m4q_noise.h"
// argv: mode seed member_base B n d state_index; prints re im per (b, component), sigma_b = 0.25 + 0.5 b
int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int mode = atoi(argv[1]);
  const unsigned long long seed = strtoull(argv[2], 0, 10), base = strtoull(argv[3], 0, 10);
  const int B = atoi(argv[4]), n = atoi(argv[5]), d = atoi(argv[6]);
  const unsigned sidx = (unsigned)atoi(argv[7]);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < n; ++c) {
      const m4q::cplx e = m4q::noise_sample(mode, seed, base + b, sidx, c, d, 0.25 + 0.5 * b);
      printf("%.17g %.17g\n", e.re, e.im);
    }
  return 0;
}
'''


def test_device_header_compiled_for_the_host_equals_the_replica(tmp_path):
    """csrc/m4q_noise.h - the code mpc_kernel and noise_sample_kernel call - built with the host compiler against a stub of the
    three device-library names it uses (__umulhi, sincospi, and <cmath>'s log / sqrt): the counter layout, the uniforms, the
    transposed and diagonal draws of the Hermitian kind and the per-member sigma against noise.py, without a device.  Same
    tolerance as on the device (tests/test_gpu_noise.py): 1e-13 on unit z, twice that for the Hermitian combination."""
    import subprocess
    clang = "/opt/rocm/lib/llvm/bin/clang++"              # the compiler the library itself is built with
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(_HIP_STUB)
    (tmp_path / "harness.cpp").write_text(_HARNESS)
    exe = str(tmp_path / "noise_host")
    subprocess.run([clang, "-O1", "-std=c++17", "-ffp-contract=off", "-I" + str(tmp_path),
                    "-I" + os.path.join(ROOT, "mpc4quantum_amd", "csrc"), str(tmp_path / "harness.cpp"), "-o", exe], check=True)
    B, seed, base = 6, 0xA4093822299F31D0, (1 << 32) - 3
    sigma = 0.25 + 0.5 * np.arange(B)
    for kind, mode in (("iid", nz.NOISE_IID), ("hermitian", nz.NOISE_HERMITIAN)):
        for n, d in ((4, 2), (9, 3), (16, 4), (8, 0)):
            if kind == "hermitian" and d == 0:
                continue
            for sidx in (1, 7):
                out = subprocess.run([exe, str(mode), str(seed), str(base), str(B), str(n), str(d), str(sidx)], check=True,
                                     capture_output=True, text=True).stdout
                a = np.array([[float(v) for v in line.split()] for line in out.strip().split("\n")])
                got = (a[:, 0] + 1j * a[:, 1]).reshape(B, n)
                want = m4q.MeasurementNoise(sigma, seed, kind, member_base=base).sample(np.arange(B), sidx, n)
                lin = 2.0 if kind == "hermitian" else 1.0
                assert np.all(np.abs(got - want) <= lin * 1e-13 * sigma[:, None]), (kind, n, sidx, np.abs(got - want).max())
                if kind == "hermitian":
                    G = got.reshape(B, d, d)
                    assert np.array_equal(G, np.conj(np.swapaxes(G, 1, 2)))

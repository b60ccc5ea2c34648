"""Observed plants on the host (no device): the definitions of mpc4quantum_amd/observe.py against the two lifts they restate, the
refusals the entry points raise before any device work, and mpc()'s choice between the device-resident loop and the host path."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs, observe as ob
from mpc4quantum_amd.distributed import mpc_batch_sharded
from mpc4quantum_amd.mpc import _runs_fused, _runs_observed, mpc_batch, open_session
from mpc4quantum_amd.session import EnsembleSession
from oracle import m4q_oracle as orc

PT, QB = ob.OBSERVE_PARTIAL_TRACE, ob.OBSERVE_QUBIT_BLOCK


def _density(rng, d, count):
    a = rng.standard_normal((count, d, d)) + 1j * rng.standard_normal((count, d, d))
    rho = a @ np.conj(np.swapaxes(a, 1, 2))
    return rho / np.trace(rho, axis1=1, axis2=2)[:, None, None]


# ---------------------------------------------------------------- 1. definitions
def test_constants_and_dims():
    assert (PT, QB) == (1, 2) == (_lib.OBSERVE_PARTIAL_TRACE, _lib.OBSERVE_QUBIT_BLOCK)
    assert ob.observe_dims(PT) == (16, 8, 4) and ob.observe_dims(QB) == (9, 4, 3)
    assert m4q.QCoupledExperiment.observe_kind == PT and m4q.QExperiment32.observe_kind == QB
    for bad in (0, 3, -1, None, "partial"):
        with pytest.raises(ValueError):
            ob.observe_dims(bad)


def test_partial_trace_equals_both_lifts_bit_for_bit():
    rng = np.random.default_rng(11)
    z = rng.standard_normal((40, 16)) + 1j * rng.standard_normal((40, 16))
    ra, rb = _density(rng, 2, 8), _density(rng, 2, 8)
    prod = np.stack([np.kron(a, b).reshape(-1) for a, b in zip(ra, rb)])
    for states in (z, prod):
        x = ob.observe_reference(PT, states)
        assert x.shape == (states.shape[0], 8)
        for b in range(states.shape[0]):
            assert np.array_equal(x[b], m4q.QCoupledExperiment.lift(states[b]))
            assert np.array_equal(x[b], orc.OracleQCoupledExperiment.lift(states[b]))
    # a product state's partial traces are its factors (unit trace each)
    assert np.abs(ob.observe_reference(PT, prod)[:, :4] - ra.reshape(-1, 4)).max() < 1e-15
    assert np.abs(ob.observe_reference(PT, prod)[:, 4:] - rb.reshape(-1, 4)).max() < 1e-15


def _block_states(rng):
    """Plant states [B, 9] for the qubit block: random three-level density matrices, rank-1 blocks, a block scaled by 1e-8."""
    rho = _density(rng, 3, 30).reshape(-1, 9)
    v = rng.standard_normal((20, 2)) + 1j * rng.standard_normal((20, 2))
    rank1 = np.zeros((20, 3, 3), dtype=complex)
    rank1[:, :2, :2] = v[:, :, None] * np.conj(v[:, None, :])
    rank1[:, 2, 2] = 0.25
    general1 = np.zeros((10, 3, 3), dtype=complex)                # rank 1 and not Hermitian: u w^H
    w = rng.standard_normal((10, 2)) + 1j * rng.standard_normal((10, 2))
    general1[:, :2, :2] = v[:10, :, None] * np.conj(w[:, None, :])
    tiny = rho[:6].copy().reshape(-1, 3, 3)
    tiny[:, :2, :2] *= 1e-8
    return np.concatenate([rho, rank1.reshape(-1, 9), general1.reshape(-1, 9), tiny.reshape(-1, 9)])


def test_qubit_block_against_the_svd_lift():
    """1e-12: the project's bound for definitions against the reference's arithmetic."""
    z = _block_states(np.random.default_rng(12))
    x = ob.observe_reference(QB, z)
    assert x.shape == (z.shape[0], 4)
    worst = 0.0
    for b in range(z.shape[0]):
        want = m4q.QExperiment32.lift(z[b])
        worst = max(worst, np.abs(x[b] - want).max() / max(1.0, np.abs(want).max()))
    print("qubit block, closed form against the SVD sum: worst %.3e" % worst)
    assert worst <= 1e-12
    # the normalised block of a density matrix has unit trace
    assert np.abs(x[:30, 0] + x[:30, 3] - 1).max() < 1e-14


def test_qubit_block_of_zero_is_nan_in_both():
    z = np.zeros((2, 9), dtype=complex)
    z[:, 8] = 1.0                                                # all the population in the third level
    assert np.all(np.isnan(ob.observe_reference(QB, z)))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.all(np.isnan(m4q.QExperiment32.lift(z[0])))


@pytest.mark.parametrize("kind, m", [(PT, 2), (QB, 1), (QB, 2)])
def test_observed_plant_step_is_plant_step_then_observe(kind, m):
    rng = np.random.default_rng(13)
    n_p, n, d = ob.observe_dims(kind)
    B = 3
    z = _density(rng, d, B).reshape(B, n_p)
    h = rng.standard_normal((B, 1 + m, d, d)) + 1j * rng.standard_normal((B, 1 + m, d, d))
    h = h + np.conj(np.swapaxes(h, -1, -2))
    u = rng.standard_normal((B, m))
    zn, xn = ob.observed_plant_step_reference(kind, z, u, h[:, 0], h[:, 1:], 0.3)
    for b in range(B):
        want = orc.plant_step(z[b], u[b], h[b, 0], list(h[b, 1:]), 0.3)
        assert np.abs(zn[b] - want).max() <= 1e-12
    assert np.array_equal(xn, ob.observe_reference(kind, zn))
    zs, _ = ob.observed_plant_step_reference(kind, z, u, h[0, 0], h[0, 1:], 0.3)         # shared operators
    assert np.array_equal(zs[0], zn[0])


# ---------------------------------------------------------------- 2. refusals before any library call
@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test."""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)


def _crosstalk_args(B=3):
    n_steps, T = 4, 6
    clock = m4q.StepClock(0.5, T, n_steps)
    z0 = np.tile(np.eye(4).reshape(1, 16) / 4, (B, 1)).astype(complex)
    args = dict(x0=z0, models=np.zeros((8, 24), dtype=complex), dim_u=2, order=1, X_targ=np.zeros((8, n_steps + T + 1)),
                U_targ=np.zeros((2, n_steps + T)), clock=clock, plant_op0=np.zeros((4, 4)), plant_ops=np.zeros((2, 4, 4)),
                Q=np.eye(8), R=np.eye(2), Qf=np.eye(8), sat=1.0)
    return args


@pytest.mark.parametrize("change", [
    dict(observe=3),
    dict(observe=QB),                                             # plant states of 16 entries are no three-level states
    dict(x0=np.zeros((3, 8), dtype=complex)),                     # the observed states instead of the plant states
    dict(x0=np.zeros(16, dtype=complex)),
    dict(plant_op0=np.zeros((2, 2))),                             # the model's operators instead of the plant's
    dict(plant_op0=np.zeros((2, 4, 4))),                          # neither shared nor one per member
    dict(plant_ops=np.zeros((3, 4, 4))),
    dict(plant_ops=np.zeros((2, 2, 4, 4))),
    dict(plant_kind=_lib.PLANT_NONE),
    dict(plant_kind=_lib.PLANT_GENERATOR),
    dict(noise=m4q.MeasurementNoise(1e-3, seed=1)),
    dict(exit_condition=m4q.QuadraticExit(np.eye(8), np.zeros(8), 0.1)),
])
def test_open_session_refuses_before_the_library(change, no_library):
    args = _crosstalk_args()
    args.setdefault("observe", PT)
    args.update(change)
    with pytest.raises(ValueError):
        open_session(**args)
    with pytest.raises(ValueError):
        mpc_batch(**args)


def test_open_session_refuses_measure_freq(no_library):
    args = _crosstalk_args()
    args["clock"].measure_freq = 2
    with pytest.raises(ValueError):
        open_session(observe=PT, **args)


def test_sharded_refuses_observe(no_library):
    args = _crosstalk_args()
    with pytest.raises(ValueError, match="observe"):
        mpc_batch_sharded(observe=PT, **args)


def _stub_session(dim_x, dim_u, plant_kind=_lib.PLANT_NONE, measure_freq=1, B=3, n_steps=4):
    """An EnsembleSession object without a library session behind it: every refusal below must come before its first use."""
    s = EnsembleSession.__new__(EnsembleSession)
    p = _lib.Problem()
    p.dim_x, p.dim_u, p.plant_kind, p.measure_freq, p.n_steps = dim_x, dim_u, plant_kind, measure_freq, n_steps
    s.problem, s.B, s.observe, s._h, s._L = p, B, 0, None, None
    return s


def test_session_methods_refuse_before_the_library(no_library):
    z0 = np.zeros((3, 16), dtype=complex)
    op0, ops = np.zeros((4, 4)), np.zeros((2, 4, 4))
    for sess, kind in ((_stub_session(8, 2, plant_kind=_lib.PLANT_HAMILTONIAN), PT), (_stub_session(8, 2, measure_freq=2), PT),
                       (_stub_session(4, 2), PT), (_stub_session(8, 2), QB), (_stub_session(8, 2), 5)):
        with pytest.raises(ValueError):
            sess.set_observed_plant(kind, op0, ops, z0)
    s = _stub_session(8, 2)
    for bad in (dict(op0=np.zeros((3, 3))), dict(ops=np.zeros((1, 4, 4))), dict(z0=np.zeros((2, 16))), dict(z0=np.zeros((3, 8)))):
        kw = dict(op0=op0, ops=ops, z0=z0)
        kw.update(bad)
        with pytest.raises(ValueError):
            s.set_observed_plant(PT, **kw)
    # without an observed plant there is nothing to run, download or restore
    for call in (lambda: s.run_observed(0, 1), s.plant_states, lambda: s.put_plant_states(np.zeros((3, 5, 16)))):
        with pytest.raises(ValueError):
            call()
    s.observe = PT
    with pytest.raises(ValueError):
        s.put_plant_states(np.zeros((3, 4, 16)))                  # n_steps + 1 = 5 columns


def test_reference_and_batch_shapes(no_library):
    for bad in (np.zeros(16), np.zeros((2, 8)), np.zeros((0, 16)), np.zeros((2, 3, 16))):
        with pytest.raises(ValueError):
            ob.observe_reference(PT, bad)
        with pytest.raises(ValueError):
            ob.observe_batch(PT, bad)
    with pytest.raises(ValueError):
        ob.observe_batch(4, np.zeros((1, 16)))


def test_capi_observe_batch_refusals():
    """m4q_observe_batch: M4Q_E_BADARG for B < 1, an unknown kind and null pointers - all before it looks for a device."""
    L = _lib.lib()
    z, zp = _lib.cbuf(np.zeros((2, 16)))
    x, xp = _lib.cbuf(np.zeros((2, 8)))
    assert L.m4q_observe_batch(0, PT, zp, xp) == _lib.E_BADARG
    assert L.m4q_observe_batch(-3, QB, zp, xp) == _lib.E_BADARG
    for kind in (0, 3, -1):
        assert L.m4q_observe_batch(2, kind, zp, xp) == _lib.E_BADARG
        assert b"observe" in L.m4q_last_error()
    assert L.m4q_observe_batch(2, PT, None, xp) == _lib.E_BADARG
    assert L.m4q_observe_batch(2, PT, zp, None) == _lib.E_BADARG
    # the session entry points refuse a null session likewise
    assert L.m4q_session_set_observed_plant(None, PT, zp, zp, 0, zp) == _lib.E_BADARG
    assert L.m4q_session_run_observed(None, 0, 1) == _lib.E_BADARG
    assert L.m4q_session_plant_states(None, zp, 16) == _lib.E_BADARG
    assert L.m4q_session_put_plant_states(None, zp, 16) == _lib.E_BADARG


# ---------------------------------------------------------------- 3. which loop mpc() runs
def _experiments():
    from mpc4quantum_amd.configs import I2, SX, SY, SZ
    coupled = lambda cls=m4q.QCoupledExperiment: cls(0.05 * np.kron(SZ, SZ), [0.5 * np.kron(SX, I2), 0.5 * np.kron(I2, SY)])   # noqa: E731
    h0 = np.diag([0.0, 1.0, 1.7]).astype(complex)
    hx = np.zeros((3, 3), dtype=complex)
    hx[0, 1] = hx[1, 0] = 0.5
    hx[1, 2] = hx[2, 1] = 0.5 * np.sqrt(2)
    leaky = lambda cls=m4q.QExperiment32: cls(h0, [hx])           # noqa: E731
    return coupled, leaky


def test_runs_observed_truth_table():
    coupled, leaky = _experiments()
    for make in (coupled, leaky):
        assert _runs_observed(make(), None, False, 1) is True
        assert _runs_observed(make(), None, False) is True
        assert not _runs_observed(make(), None, False, 2)                          # measure_freq
        assert not _runs_observed(make(), None, True, 1)                           # streaming
        assert not _runs_observed(make(), lambda xn, x, u: False, False, 1)        # a host exit condition
        assert not _runs_observed(make(), m4q.QuadraticExit(np.eye(4), np.zeros(4), 0.1), False, 1)
        e = make()
        e.set_sigma(1e-3)
        assert not _runs_observed(e, None, False, 1)
        e = make()
        e.set_noise(m4q.MeasurementNoise(1e-3, seed=3))
        assert not _runs_observed(e, None, False, 1)
        e = make()
        e.set("c_ops", [np.eye(e.H0.shape[0])])
        assert not _runs_observed(e, None, False, 1)
        e = make()
        e.set("e_ops", [np.eye(e.H0.shape[0])])
        assert not _runs_observed(e, None, False, 1)
        e = make()
        e.set("options", {"nsteps": 1000})                                          # (only tunes the reference's integrator)
        assert _runs_observed(e, None, False, 1) is True

    class OwnLift(m4q.QCoupledExperiment):
        @staticmethod
        def lift(v):
            return m4q.QCoupledExperiment.lift(v)

    class Plain32(m4q.QExperiment32):
        pass

    assert not _runs_observed(coupled(OwnLift), None, False, 1)                    # a subclass may bring its own lift
    assert not _runs_observed(leaky(Plain32), None, False, 1)                      # exactly the two classes
    p = configs.build(1, batch=1)
    assert not _runs_observed(m4q.QExperiment(p["plant_op0"][0], list(p["plant_ops"][0])), None, False, 1)
    assert not _runs_observed(orc.OracleQCoupledExperiment(np.eye(4), [np.eye(4)]), None, False, 1)
    # two qutrits: the same class, not the dimensions the kernels are built for
    assert not _runs_observed(m4q.QCoupledExperiment(np.eye(9), [np.eye(9)]), None, False, 1)
    # the fused predicate is what it was
    assert not _runs_fused(coupled(), None, False) and not _runs_fused(leaky(), None, False)

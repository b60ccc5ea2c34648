"""CPU checks of the open-loop rollouts (m4q_plant_rollout_batch, m4q_model_rollout_batch; mpc4quantum_amd/rollout.py): every
refusal of the C ABI comes back with its code before a device is asked for, the Python wrappers refuse every mismatched shape
before the library is touched, and a time grid becomes the interval lengths the kernel integrates over."""
import ctypes

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, rollout

DP = _lib._dp


def _buf(n):
    a = np.zeros(max(int(n), 1), dtype=np.float64)
    return a, a.ctypes.data_as(DP)


class _PlantCall:
    """One valid m4q_plant_rollout_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, N=4, k=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, kind=kind, N=N, dts=self._b("dts", N), x0=self._b("x0", 2 * B * n), u=self._b("u", N * m), u_per=0,
                      u_scale=None, op0=self._b("op0", 2 * k * k), ops=self._b("ops", 2 * m * k * k), per=0, W=self._b("W", 2 * n * n),
                      target=self._b("f", 2 * n), t_per=0, xs_mode=2, xs=self._b("xs", 2 * B * (N + 1) * n), q_mode=2,
                      q=self._b("q", B * (N + 1)))

    def _b(self, name, count):
        self.keep[name], p = _buf(count)
        return p

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_rollout_batch(v["B"], v["n"], v["m"], v["kind"], v["N"], v["dts"], v["x0"], v["u"], v["u_per"],
                                                  v["u_scale"], v["op0"], v["ops"], v["per"], v["W"], v["target"], v["t_per"],
                                                  v["xs_mode"], v["xs"], v["q_mode"], v["q"])


class _ModelCall:
    def __init__(self, B=3, n=9, m=2, order=1, N=4, P=2):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, order=order, N=N, x0=self._b("x0", 2 * B * n), u=self._b("u", N * m), u_per=0, u_scale=None,
                      models=self._b("models", 2 * n * n * (1 + P)), m_per=0, W=self._b("W", 2 * n * n), target=self._b("f", 2 * n),
                      t_per=0, xs_mode=2, xs=self._b("xs", 2 * B * (N + 1) * n), q_mode=2, q=self._b("q", B * (N + 1)))

    _b = _PlantCall._b

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_model_rollout_batch(v["B"], v["n"], v["m"], v["order"], v["N"], v["x0"], v["u"], v["u_per"], v["u_scale"],
                                                  v["models"], v["m_per"], v["W"], v["target"], v["t_per"], v["xs_mode"], v["xs"],
                                                  v["q_mode"], v["q"])


BAD_COMMON = [dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(x0=None), dict(u=None), dict(xs=None), dict(q=None),
              dict(xs_mode=3), dict(xs_mode=-1), dict(q_mode=3), dict(q_mode=-1), dict(xs_mode=0, q_mode=0),
              dict(W=None), dict(target=None), dict(q_mode=1, W=None), dict(q_mode=1, target=None)]


@pytest.mark.parametrize("change", BAD_COMMON + [dict(dts=None), dict(op0=None), dict(ops=None), dict(kind=0), dict(kind=4),
                                                 dict(kind=-1), dict(kind=_lib.PLANT_PROCESS)], ids=str)
def test_plant_rollout_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _PlantCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", BAD_COMMON + [dict(models=None)], ids=str)
def test_model_rollout_refuses_bad_arguments(change):
    assert _ModelCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_rollouts_refuse_shapes_without_a_kernel():
    assert _PlantCall(n=25, k=5)() == _lib.E_UNSUPPORTED                       # no compiled shape
    assert _PlantCall(n=9, m=3)() == _lib.E_UNSUPPORTED
    assert _PlantCall(n=8, m=2, k=2)() == _lib.E_UNSUPPORTED                   # a shape with a model and no device plant
    assert _ModelCall(n=25, P=2)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED         # the plant-only shape has no model kernel


def test_unused_optional_arrays_may_be_null():
    """Without a figure W and target are not read; without states xs is not: such calls get as far as asking for a device."""
    ok = (0, _lib.E_NODEVICE)
    assert _PlantCall()(q_mode=0, W=None, target=None, q=None) in ok
    assert _PlantCall()(xs_mode=0, xs=None) in ok
    assert _ModelCall()(q_mode=0, W=None, target=None, q=None) in ok
    assert _ModelCall()(xs_mode=0, xs=None) in ok


def test_valid_calls_need_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _PlantCall()() == _lib.E_NODEVICE
    assert _PlantCall(n=16, m=2, k=4)() == _lib.E_NODEVICE                    # the plant-only shape serves the plant rollout
    assert _PlantCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2)() == _lib.E_NODEVICE
    assert _PlantCall(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_NODEVICE
    assert _ModelCall()() == _lib.E_NODEVICE
    assert _ModelCall(n=8, m=2)() == _lib.E_NODEVICE
    assert _ModelCall(n=16, m=1, order=4, P=4)() == _lib.E_NODEVICE
    with pytest.raises(_lib.M4qError):
        m4q.plant_rollout_batch(np.zeros((1, 4)), np.zeros((3, 1)), np.eye(2), np.eye(2)[None], 0.1)
    with pytest.raises(_lib.M4qError):
        m4q.model_rollout_batch(np.zeros((1, 4)), np.zeros((3, 1)), np.zeros((4, 8)), 1)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _plant_args(B=3, n=9, m=2, N=4, k=3):
    return dict(x0=np.zeros((B, n), complex), us=np.zeros((N, m)), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex),
                dt_or_ts=0.25)


PLANT_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((3, 9, 1))), dict(x0=np.zeros((0, 9))),
             dict(us=np.zeros(4)), dict(us=np.zeros((2, 4, 2))), dict(us=np.zeros((3, 4, 2, 1))), dict(us=np.zeros((0, 2))),
             dict(op0=np.zeros((2, 2))), dict(op0=np.zeros((2, 3, 3))), dict(op0=np.zeros((9, 9))), dict(op0=np.zeros((1, 1, 3, 3))),
             dict(ops=np.zeros((3, 3))), dict(ops=np.zeros((1, 3, 3))), dict(ops=np.zeros((2, 2, 3, 3))), dict(ops=np.zeros((2, 2, 2))),
             dict(dt_or_ts=np.zeros(4)), dict(dt_or_ts=np.zeros(6)), dict(dt_or_ts=np.zeros((5, 1))), dict(dt_or_ts=np.inf),
             dict(u_scale=np.ones(2)), dict(u_scale=np.ones((3, 1))), dict(u_scale=np.ones((2, 2))),
             dict(kind=0), dict(kind=7), dict(kind=_lib.PLANT_PROCESS), dict(kind=_lib.PLANT_GENERATOR),
             dict(keep="first"), dict(figure="sum"), dict(keep="none"), dict(figure="all"), dict(figure="last", W=np.eye(9)),
             dict(figure="last", target=np.zeros(9)), dict(figure="all", W=np.eye(4), target=np.zeros(9)),
             dict(figure="all", W=np.eye(9), target=np.zeros(4)), dict(figure="all", W=np.eye(9), target=np.zeros((2, 9))),
             dict(figure="all", W=np.zeros((1, 9, 9)), target=np.zeros(9))]


@pytest.mark.parametrize("change", PLANT_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_plant_rollout_wrapper_refuses_bad_shapes(no_library, change):
    """(kind = GENERATOR / PROCESS with the Hamiltonian's 3 x 3 operators: wrong operator size for that plant.)"""
    with pytest.raises(ValueError):
        m4q.plant_rollout_batch(**dict(_plant_args(), **change))


def test_plant_rollout_wrapper_refuses_non_square_states(no_library):
    with pytest.raises(ValueError):
        m4q.plant_rollout_batch(**_plant_args(n=8, k=2))
    with pytest.raises(ValueError):
        m4q.plant_rollout_batch(**dict(_plant_args(n=8, k=8), kind=_lib.PLANT_GENERATOR))


MODEL_BAD = [dict(x0=np.zeros(9)), dict(us=np.zeros(4)), dict(us=np.zeros((2, 4, 2))), dict(models=np.zeros((9, 18))),
             dict(models=np.zeros((2, 9, 27))), dict(models=np.zeros((9, 9, 3))), dict(models=np.zeros(27)), dict(order=2), dict(order=0),
             dict(u_scale=np.ones((3, 3))), dict(keep="none"), dict(figure="last"), dict(figure="all", W=np.eye(9), target=np.zeros(8)),
             dict(keep="every")]


@pytest.mark.parametrize("change", MODEL_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items()))
def test_model_rollout_wrapper_refuses_bad_shapes(no_library, change):
    args = dict(x0=np.zeros((3, 9), complex), us=np.zeros((4, 2)), models=np.zeros((9, 27), complex), order=1)
    with pytest.raises(ValueError):
        m4q.model_rollout_batch(**dict(args, **change))


def test_simulate_batch_refuses_bad_controls(no_library):
    H0, Hk = np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)]
    ts = np.arange(5) * 0.25
    x0 = np.zeros((3, 9), complex)
    for exp in (m4q.QExperiment(H0, Hk), m4q.LExperiment(np.eye(9), [np.eye(9)] * 2)):
        for us in (np.zeros((3, 5)), np.zeros((2, 3)), np.zeros((2, 2, 5)), np.zeros((3, 2, 3))):
            with pytest.raises(ValueError):
                exp.simulate_batch(x0, ts, us)
        with pytest.raises(ValueError):
            exp.simulate_batch(x0, ts[:1], np.zeros((2, 5)))
        with pytest.raises(ValueError):
            exp.simulate_batch(x0, ts, np.zeros((2, 5)), op0=np.zeros((2, 3, 3)))
    syn = m4q.QSynthesis(np.zeros((2, 2)), [np.eye(2)])
    with pytest.raises(ValueError):
        syn.simulate_batch(np.zeros((3, 9), complex), ts, np.zeros((1, 5)))       # 9 is no fourth power


# ---------------------------------------------------------------- ts -> dts, held controls
def test_time_grid_becomes_interval_lengths():
    assert np.array_equal(rollout.dts_of(0.25, 3), [0.25, 0.25, 0.25])
    assert np.array_equal(rollout.dts_of(np.float64(0.5), 1), [0.5])
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    dts = rollout.dts_of(ts, 4)
    assert dts.dtype == np.float64 and dts.flags["C_CONTIGUOUS"]
    assert np.array_equal(dts, [ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2], ts[4] - ts[3]])     # the very subtractions simulate() makes
    assert np.array_equal(rollout.dts_of(list(ts + 3.0), 4), np.diff(ts + 3.0))
    assert np.array_equal(rollout.dts_of(np.arange(4), 3), [1.0, 1.0, 1.0])                      # an integer grid


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    """The arguments of the C call for a non-uniform grid, a shared sequence, per-member op0 beside shared control operators, a
    per-member target: interval lengths, strides flags and modes as the ABI reads them."""
    seen = {}

    class Fake:
        def m4q_plant_rollout_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N = 3, 9, 2, 4
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    us = np.arange(N * m, dtype=float).reshape(N, m)
    op0 = np.arange(B * 9).reshape(B, 3, 3)
    ops = np.ones((m, 3, 3))
    out = m4q.plant_rollout_batch(np.zeros((B, n)), us, op0, ops, ts, u_scale=np.ones((B, m)), W=np.eye(n), target=np.zeros((B, n)),
                                  keep="last", figure="all")
    a = seen["a"]
    assert a[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N)
    assert np.array_equal(np.ctypeslib.as_array(a[5], (N,)), np.diff(ts))
    assert np.array_equal(np.ctypeslib.as_array(a[7], (N * m,)), us.reshape(-1)) and a[8] == 0 and a[9] is not None
    assert a[12] == 1                                                                   # per-member operators ...
    assert np.array_equal(np.ctypeslib.as_array(a[11], (B * m * 9 * 2,))[::2], np.ones(B * m * 9))  # ... the shared set repeated
    assert a[15] == 1 and a[16] == 1 and a[18] == 2
    assert out["xs"].shape == (B, n) and out["q"].shape == (B, N + 1)
    out = m4q.plant_rollout_batch(np.zeros((B, n)), np.zeros((B, N, m)), op0[0], ops, 0.5, keep="all")
    a = seen["a"]
    assert a[8] == 1 and a[9] is None and a[12] == 0 and a[13] is None and a[14] is None and a[16] == 2 and a[18] == 0 and a[19] is None
    assert np.array_equal(np.ctypeslib.as_array(a[5], (N,)), [0.5] * N)
    assert set(out) == {"xs"} and out["xs"].shape == (B, N + 1, n)


def test_held_controls_follow_simulate():
    """Column i of an (m, len(ts)) array is held on [ts[i], ts[i + 1]); a callable is sampled at ts[i]; the last column is unused."""
    ts = np.array([0.0, 0.5, 0.6, 2.0])
    us = np.arange(8, dtype=float).reshape(2, 4)
    assert np.array_equal(rollout.held_controls(us, ts, 2, 5), us[:, :3].T)
    assert np.array_equal(rollout.held_controls(us[:, :3], ts, 2, 5), us[:, :3].T)
    assert np.array_equal(rollout.held_controls(lambda t: [t, -t], ts, 2, 5), np.stack([ts[:3], -ts[:3]], axis=1))
    per = np.arange(40, dtype=float).reshape(5, 2, 4)
    got = rollout.held_controls(per, ts, 2, 5)
    assert got.shape == (5, 3, 2) and np.array_equal(got[4, 1], per[4, :, 1])
    assert rollout.held_controls(np.arange(4.0), ts, 1, 5).shape == (3, 1)


def test_prototypes_and_exports():
    assert "m4q_plant_rollout_batch" in _lib.PROTOTYPES and "m4q_model_rollout_batch" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["m4q_plant_rollout_batch"][1]) == 20 and len(_lib.PROTOTYPES["m4q_model_rollout_batch"][1]) == 18
    assert m4q.plant_rollout_batch is rollout.plant_rollout_batch and m4q.model_rollout_batch is rollout.model_rollout_batch
    for cls in (m4q.QExperiment, m4q.LExperiment, m4q.QSynthesis):
        assert callable(cls.simulate_batch)
    assert ctypes.sizeof(ctypes.c_double) == 8

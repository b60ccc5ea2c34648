"""CPU checks of the rollout gradients (m4q_plant_rollout_grad_batch, m4q_model_rollout_grad_batch; mpc4quantum_amd/grad.py): the
NumPy / SciPy definitions against central differences of an independent forward chain, the ordered ensemble sum, every refusal of
the C ABI before a device is asked for and every ValueError of the Python wrappers before the library is touched."""
import math

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, grad
from tests import grad_cases as gc

DP = _lib._dp
H_FD = 1e-5
# central differences with h = 1e-5 carry an h^2 f''' / 6 term and rounding of about eps |J| / h ~ 1e-10: agreement was at most
# 9.5e-10 of max(1, max|g|) when the formulas were first checked; the bound is 100 times that
FD_BOUND = 1e-7
N_FD, B_FD = 5, 2


def _central(J, p):
    """dJ/dp [B, *p.shape] of J(p) -> [B] by central differences, entry by entry."""
    g = np.empty((B_FD,) + p.shape)
    for idx in np.ndindex(*p.shape):
        hi, lo = p.copy(), p.copy()
        hi[idx] += H_FD
        lo[idx] -= H_FD
        g[(slice(None),) + idx] = (J(hi) - J(lo)) / (2 * H_FD)
    return g


def _objective(q, figure):
    return q[:, -1] if figure == "last" else q.sum(axis=1)


def _check(ref, J_of, u, sc, figure, q_chain):
    # the reference's forward figure against the chained independent steps
    q_ref = ref["q"] if figure == "sum" else ref["q"][:, None]
    q_ind = q_chain if figure == "sum" else q_chain[:, -1:]
    assert np.abs(q_ref - q_ind).max() <= 1e-12 * max(1.0, np.abs(q_ind).max())
    g_u = _central(lambda p: J_of(p, sc), u)
    g_all = _central(lambda p: J_of(u, p), sc)                    # [member, whose scale, k]
    g_s = np.stack([g_all[b, b] for b in range(B_FD)])
    assert all(np.all(g_all[b, a] == 0.0) for b in range(B_FD) for a in range(B_FD) if a != b)   # a member sees its own scales alone
    for name, got, fd in (("grad", ref["grad"], g_u), ("grad_scale", ref["grad_scale"], g_s)):
        err = np.abs(got - fd).max() / max(1.0, np.abs(got).max())
        print("%s: max|g| = %.3e, against central differences %.2e" % (name, np.abs(got).max(), err))
        assert got.shape == fd.shape and err <= FD_BOUND
        assert np.abs(got).max() > 1e-3                            # (a gradient that vanishes would prove nothing)


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("name", gc.PLANT_NAMES)
def test_plant_reference_against_central_differences(name, figure):
    c = gc.plant_case(name)
    rng = np.random.default_rng(9000 + 17 * gc.PLANT_NAMES.index(name) + (1 if figure == "sum" else 0))
    x0 = c.states(rng, B_FD)
    op0, ops = c.member_ops(rng, B_FD)
    u = rng.uniform(-c.sat, c.sat, (N_FD, c.m))
    sc = 1 + 0.1 * rng.standard_normal((B_FD, c.m))
    W, f = gc.weights_and_targets(rng, c.n, B_FD)
    ts = gc.grid(rng, N_FD, c.dt)

    def q_of(uu, ss):
        xs = np.stack([gc.plant_chain(c, x0[b], ss[b][None, :] * uu, op0[b], ops[b], np.diff(ts)) for b in range(B_FD)])
        return gc.figures(xs, W, f)
    ref = m4q.plant_rollout_grad_reference(x0, u, op0, ops, ts, W, f, c.kind, u_scale=sc, figure=figure)
    _check(ref, lambda uu, ss: _objective(q_of(uu, ss), figure), u, sc, figure, q_of(u, sc))


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("shape", [(4, 1, 2), (9, 2, 2), (8, 2, 1), (16, 1, 4)], ids=lambda s: "%d-%d-%d" % s)
def test_model_reference_against_central_differences(shape, figure):
    n, m, order = shape
    models, x0, sat, rng = gc.model_case(n, m, order, B_FD, 9100 + 100 * n + 10 * m + order)
    u = rng.uniform(-sat, sat, (N_FD, m))
    sc = 1 + 0.1 * rng.standard_normal((B_FD, m))
    W, f = gc.weights_and_targets(rng, n, B_FD)

    def q_of(uu, ss):
        xs = np.stack([gc.model_chain(models[b], m, order, x0[b], ss[b][None, :] * uu) for b in range(B_FD)])
        return gc.figures(xs, W, f)
    ref = m4q.model_rollout_grad_reference(x0, u, models, order, W, f, u_scale=sc, figure=figure)
    _check(ref, lambda uu, ss: _objective(q_of(uu, ss), figure), u, sc, figure, q_of(u, sc))


def test_reference_with_per_member_sequences_and_shared_data():
    """Per-member control sequences, one operator set, one target, a scalar dt, no u_scale: each member is a call of its own."""
    c = gc.plant_case("4-2")
    rng = np.random.default_rng(9200)
    B, N = 3, 4
    x0 = c.states(rng, B)
    u = rng.uniform(-c.sat, c.sat, (B, N, c.m))
    W, f = gc.weights_and_targets(rng, c.n, 1)
    ref = m4q.plant_rollout_grad_reference(x0, u, c.op0, c.ops, c.dt, W, f[0], figure="sum")
    assert ref["q"].shape == (B, N + 1) and ref["grad"].shape == (B, N, c.m) and ref["grad_scale"].shape == (B, c.m)
    for b in range(B):
        one = m4q.plant_rollout_grad_reference(x0[b:b + 1], u[b], c.op0, c.ops, c.dt, W, f, figure="sum")
        assert np.array_equal(one["grad"][0], ref["grad"][b]) and np.array_equal(one["q"][0], ref["q"][b])
    # with u_scale absent the derivative with respect to a scale of 1 is sum_t u[t][k] grad[t][k]
    assert np.allclose(ref["grad_scale"], (u * ref["grad"]).sum(axis=1), rtol=1e-12, atol=1e-15)
    red = m4q.plant_rollout_grad_reference(x0, u[0], c.op0, c.ops, c.dt, W, f[0], figure="sum", reduce=True, weights=[0.2, 0.3, 0.5])
    full = m4q.plant_rollout_grad_reference(x0, u[0], c.op0, c.ops, c.dt, W, f[0], figure="sum")
    assert red["grad"].shape == (N, c.m)
    assert np.array_equal(red["grad"], m4q.ordered_weighted_sum(full["grad"], [0.2, 0.3, 0.5]))
    J = np.zeros(B)
    for t in range(N + 1):
        J = J + full["q"][:, t]
    assert red["q_mean"] == m4q.ordered_weighted_sum(J, [0.2, 0.3, 0.5])


# ---------------------------------------------------------------- the ordered sum
def test_ordered_weighted_sum_against_fsum():
    """B = 1,030: five chunks, the last ragged.  Positive terms: a sequential sum of at most 256 + 5 additions is within
    261 eps / 2 = 2.9e-14 of the exact sum of the rounded products, relative to it."""
    rng = np.random.default_rng(9300)
    B = 1030
    v = rng.uniform(0.5, 1.5, (B, 3))
    w = rng.uniform(0.0, 2.0, B)
    for weights, ws in ((w, w), (None, np.full(B, 1.0 / B))):
        got = m4q.ordered_weighted_sum(v, weights)
        for e in range(3):
            exact = math.fsum(ws[b] * v[b, e] for b in range(B))
            assert abs(got[e] - exact) <= 1e-13 * abs(exact)
    assert m4q.ordered_weighted_sum(v[:, 0], w).shape == ()
    with pytest.raises(ValueError):
        m4q.ordered_weighted_sum(v, w[:-1])
    with pytest.raises(ValueError):
        m4q.ordered_weighted_sum(np.zeros((0, 3)))


def test_ordered_weighted_sum_keeps_its_stated_order():
    """Three chunks (256, 256, 88) of a hand-made sequence whose sum depends on the order: 1.0 first, then 2^-53 599 times.
    Chunk 0: 1 + 2^-53 is a tie and rounds to even, 255 times: 1.0.  Chunk 1: 256 2^-53 = 2^-45.  Chunk 2: 88 2^-53 = 44 2^-52.
    The partials are added in turn, each sum exact: 1 + 2^-45 + 44 2^-52.  (The exact sum is 1 + 599 2^-53.)"""
    tiny = 2.0 ** -53
    v = np.full(600, tiny)
    v[0] = 1.0
    ones = np.ones(600)
    assert m4q.ordered_weighted_sum(v, ones) == 1.0 + 2.0 ** -45 + 44 * 2.0 ** -52
    # the same numbers with the 1.0 last in its chunk: 255 2^-53 + 1 = 1 + 127.5 2^-52, a tie that rounds to 1 + 128 2^-52
    p = v.copy()
    p[0], p[255] = tiny, 1.0
    assert m4q.ordered_weighted_sum(p, ones) == (1.0 + 128 * 2.0 ** -52) + 2.0 ** -45 + 44 * 2.0 ** -52
    assert m4q.ordered_weighted_sum(p, ones) != m4q.ordered_weighted_sum(v, ones)
    # the product is rounded before it is added: 3 (1/3) = 1.0 exactly only because 1/3 is rounded first
    assert m4q.ordered_weighted_sum(np.array([3.0, 3.0]), np.array([1.0 / 3.0, 1.0 / 3.0])) == 2.0


# ---------------------------------------------------------------- the C entry points
def _buf(n):
    a = np.zeros(max(int(n), 1), dtype=np.float64)
    return a, a.ctypes.data_as(DP)


class _PlantCall:
    """One valid m4q_plant_rollout_grad_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, N=4, k=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, kind=kind, N=N, dts=self._b("dts", N), x0=self._b("x0", 2 * B * n), u=self._b("u", B * N * m), u_per=0,
                      u_scale=None, op0=self._b("op0", 2 * k * k), ops=self._b("ops", 2 * m * k * k), per=0, W=self._b("W", 2 * n * n),
                      target=self._b("f", 2 * n), t_per=0, q_mode=2, weights=None, reduce=0, q=self._b("q", B * (N + 1)),
                      grad=self._b("grad", B * N * m), grad_scale=self._b("gs", B * m), q_mean=self._b("qm", 1))

    def _b(self, name, count):
        self.keep[name], p = _buf(count)
        return p

    def weights(self, values):
        self.keep["w"] = np.array(values, dtype=np.float64)
        return self.keep["w"].ctypes.data_as(DP)

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_rollout_grad_batch(v["B"], v["n"], v["m"], v["kind"], v["N"], v["dts"], v["x0"], v["u"], v["u_per"],
                                                       v["u_scale"], v["op0"], v["ops"], v["per"], v["W"], v["target"], v["t_per"],
                                                       v["q_mode"], v["weights"], v["reduce"], v["q"], v["grad"], v["grad_scale"],
                                                       v["q_mean"])


class _ModelCall:
    def __init__(self, B=3, n=9, m=2, order=1, N=4, P=2):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, order=order, N=N, x0=self._b("x0", 2 * B * n), u=self._b("u", B * N * m), u_per=0, u_scale=None,
                      models=self._b("models", 2 * n * n * (1 + P)), m_per=0, W=self._b("W", 2 * n * n), target=self._b("f", 2 * n),
                      t_per=0, q_mode=2, weights=None, reduce=0, q=self._b("q", B * (N + 1)), grad=self._b("grad", B * N * m),
                      grad_scale=self._b("gs", B * m), q_mean=self._b("qm", 1))

    _b = _PlantCall._b
    weights = _PlantCall.weights

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_model_rollout_grad_batch(v["B"], v["n"], v["m"], v["order"], v["N"], v["x0"], v["u"], v["u_per"],
                                                       v["u_scale"], v["models"], v["m_per"], v["W"], v["target"], v["t_per"], v["q_mode"],
                                                       v["weights"], v["reduce"], v["q"], v["grad"], v["grad_scale"], v["q_mean"])


BAD_COMMON = [dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(x0=None), dict(u=None), dict(W=None), dict(target=None), dict(q=None),
              dict(grad=None), dict(q_mode=0), dict(q_mode=3), dict(q_mode=-1), dict(reduce=1, u_per=1), dict(reduce=1, q_mean=None)]
BAD_WEIGHTS = [[1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -1e-300], [-1.0, 1.0, 1.0]]


@pytest.mark.parametrize("change", BAD_COMMON + [dict(dts=None), dict(op0=None), dict(ops=None), dict(kind=0), dict(kind=4),
                                                 dict(kind=-1), dict(kind=_lib.PLANT_PROCESS)], ids=str)
def test_plant_gradient_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _PlantCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", BAD_COMMON + [dict(models=None)], ids=str)
def test_model_gradient_refuses_bad_arguments(change):
    assert _ModelCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


@pytest.mark.parametrize("values", BAD_WEIGHTS, ids=str)
@pytest.mark.parametrize("reduce", [0, 1])
def test_gradients_refuse_bad_weights(values, reduce):
    for call in (_PlantCall(), _ModelCall()):
        assert call(weights=call.weights(values), reduce=reduce) == _lib.E_BADARG


def test_gradients_refuse_what_has_no_kernel():
    assert _PlantCall(n=25, k=5)() == _lib.E_UNSUPPORTED                       # no compiled shape
    assert _PlantCall(n=9, m=3)() == _lib.E_UNSUPPORTED
    assert _PlantCall(n=8, m=2, k=2)() == _lib.E_UNSUPPORTED                   # a shape with a model and no device plant
    assert _PlantCall(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_UNSUPPORTED          # the generator plant
    assert b"generator" in _lib.lib().m4q_last_error() and b"m4q_model_rollout_grad_batch" in _lib.lib().m4q_last_error()
    assert _PlantCall(n=4, m=1, kind=_lib.PLANT_GENERATOR, k=4)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=25, P=2)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=9, order=3, P=9)() == _lib.E_UNSUPPORTED
    assert _ModelCall(n=16, m=2, order=1, P=2)() == _lib.E_UNSUPPORTED         # the plant-only shape has no model kernel


def test_well_formed_calls_reach_the_device():
    """Every check passed: the call asks for a device (and, where there is one, runs on the all-zero data)."""
    want = 0 if _lib.device_count() > 0 else _lib.E_NODEVICE
    assert _PlantCall()() == want
    assert _PlantCall()(q_mode=1, grad_scale=None) == want
    p = _PlantCall()
    assert p(reduce=1, weights=p.weights([0.0, 1.0, 2.5])) == want
    assert _PlantCall()(reduce=1) == want
    assert _PlantCall(n=16, m=2, k=4)() == want                               # the plant-only shape serves the plant gradient
    assert _PlantCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2)() == want
    assert _ModelCall()() == want
    assert _ModelCall()(reduce=1, grad_scale=None) == want
    assert _ModelCall(n=8, m=2)() == want
    assert _ModelCall(n=16, m=1, order=4, P=4)() == want


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _plant_args(B=3, n=9, m=2, N=4, k=3):
    return dict(x0=np.zeros((B, n), complex), us=np.zeros((N, m)), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex),
                dt_or_ts=0.25, W=np.eye(n), target=np.zeros(n))


COMMON_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((0, 9))), dict(us=np.zeros(4)), dict(us=np.zeros((2, 4, 2))),
              dict(u_scale=np.ones((3, 1))), dict(u_scale=np.ones(2)), dict(W=None), dict(target=None), dict(W=np.eye(4)),
              dict(W=np.zeros((1, 9, 9))), dict(target=np.zeros(4)), dict(target=np.zeros((2, 9))),
              dict(figure="all"), dict(figure="none"), dict(figure=1),
              dict(reduce=True, us=np.zeros((3, 4, 2))), dict(reduce=True, weights=np.ones(2)), dict(reduce=True, weights=np.ones((3, 1))),
              dict(reduce=True, weights=[1.0, np.nan, 1.0]), dict(reduce=True, weights=[1.0, -1.0, 1.0]),
              dict(reduce=True, weights=[1.0, np.inf, 1.0]), dict(weights=np.ones(2)), dict(weights=[1.0, -1.0, 1.0])]   # (without reduce the weights are checked and otherwise unused)
PLANT_BAD = COMMON_BAD + [dict(op0=np.zeros((2, 2))), dict(op0=np.zeros((2, 3, 3))), dict(ops=np.zeros((3, 3))),
                          dict(ops=np.zeros((1, 3, 3))), dict(ops=np.zeros((2, 2, 3, 3))), dict(dt_or_ts=np.zeros(4)),
                          dict(dt_or_ts=np.inf), dict(kind=0), dict(kind=7), dict(kind=_lib.PLANT_PROCESS),
                          dict(kind=_lib.PLANT_GENERATOR)]


def _ident(c):
    return ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items())


@pytest.mark.parametrize("change", PLANT_BAD, ids=_ident)
def test_plant_gradient_wrapper_refuses_bad_arguments(no_library, change):
    """(kind = GENERATOR / PROCESS with the Hamiltonian's 3 x 3 operators: wrong operator size for that plant.)"""
    with pytest.raises(ValueError):
        m4q.plant_rollout_grad_batch(**dict(_plant_args(), **change))
    if "kind" not in change and "dt_or_ts" not in change:
        with pytest.raises(ValueError):
            m4q.plant_rollout_grad_reference(**dict(_plant_args(), **change))


@pytest.mark.parametrize("change", COMMON_BAD + [dict(models=np.zeros((9, 18))), dict(models=np.zeros((2, 9, 27))), dict(models=np.zeros(27)),
                                                 dict(order=2), dict(order=0)], ids=_ident)
def test_model_gradient_wrapper_refuses_bad_arguments(no_library, change):
    args = dict(x0=np.zeros((3, 9), complex), us=np.zeros((4, 2)), models=np.zeros((9, 27), complex), order=1, W=np.eye(9),
                target=np.zeros(9))
    with pytest.raises(ValueError):
        m4q.model_rollout_grad_batch(**dict(args, **change))
    with pytest.raises(ValueError):
        m4q.model_rollout_grad_reference(**dict(args, **change))


def test_experiment_wrappers_refuse_before_the_library(no_library):
    ts = np.arange(5) * 0.25
    x0 = np.zeros((3, 9), complex)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    for us in (np.zeros((3, 5)), np.zeros((2, 3)), np.zeros((2, 2, 5))):
        with pytest.raises(ValueError):
            exp.gradient_batch(x0, ts, us, np.eye(9), np.zeros(9))
    with pytest.raises(ValueError):
        exp.gradient_batch(x0, ts, np.zeros((2, 5)), np.eye(9), np.zeros(9), figure="all")
    with pytest.raises(ValueError, match="model_rollout_grad_batch"):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).gradient_batch(x0, ts, np.zeros((2, 5)), np.eye(9), np.zeros(9))
    with pytest.raises(ValueError):
        m4q.QSynthesis(np.zeros((2, 2)), [np.eye(2)]).gradient_batch(x0, ts, np.zeros((1, 5)), np.eye(9), np.zeros(9))   # 9 is no fourth power


def test_wrapper_hands_the_kernel_what_it_was_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_plant_rollout_grad_batch(self, *a):
            seen["a"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N = 3, 9, 2, 4
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    us = np.arange(N * m, dtype=float).reshape(N, m)
    op0 = np.arange(B * 9).reshape(B, 3, 3)
    out = m4q.plant_rollout_grad_batch(np.zeros((B, n)), us, op0, np.ones((m, 3, 3)), ts, np.eye(n), np.zeros((B, n)), u_scale=np.ones((B, m)),
                                       figure="sum", weights=[1.0, 2.0, 3.0], reduce=True, scale_grad=True)
    a = seen["a"]
    assert len(a) == 23 and a[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N)
    assert np.array_equal(np.ctypeslib.as_array(a[5], (N,)), np.diff(ts))
    assert a[8] == 0 and a[9] is not None and a[12] == 1 and a[15] == 1 and a[16] == 2 and a[18] == 1
    assert np.array_equal(np.ctypeslib.as_array(a[17], (B,)), [1.0, 2.0, 3.0])
    assert out["q"].shape == (B, N + 1) and out["grad"].shape == (N, m) and out["grad_scale"].shape == (B, m) and isinstance(out["q_mean"], float)
    out = m4q.plant_rollout_grad_batch(np.zeros((B, n)), np.zeros((B, N, m)), op0[0], np.ones((m, 3, 3)), 0.5, np.eye(n), np.zeros(n))
    a = seen["a"]
    assert a[8] == 1 and a[9] is None and a[12] == 0 and a[15] == 0 and a[16] == 1 and a[17] is None and a[18] == 0
    assert a[21] is None and a[22] is None
    assert set(out) == {"q", "grad"} and out["q"].shape == (B,) and out["grad"].shape == (B, N, m)


def test_prototypes_and_exports():
    assert len(_lib.PROTOTYPES["m4q_plant_rollout_grad_batch"][1]) == 23 and len(_lib.PROTOTYPES["m4q_model_rollout_grad_batch"][1]) == 21
    assert m4q.plant_rollout_grad_batch is grad.plant_rollout_grad_batch and m4q.model_rollout_grad_batch is grad.model_rollout_grad_batch
    for cls in (m4q.QExperiment, m4q.LExperiment, m4q.QSynthesis):
        assert callable(cls.gradient_batch)

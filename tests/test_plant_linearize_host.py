"""CPU checks of the plant's own linearisation (m4q_plant_linearize_batch; mpc4quantum_amd/plant_linearize.py): the NumPy / SciPy
definition against the independent plant step - exactness at the point, central differences for B, a second-order remainder -
every refusal of the C ABI with its code before a device is asked for, and the Python wrappers' refusals before the library is
touched."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, plant_linearize
from tests import grad_cases as gc
from tests.test_grad_host import FD_BOUND, H_FD

DP = _lib._dp
PLANTS = gc.PLANT_NAMES + ("16-2",)                                # the six cases and the plant-only shape
B_DEF, T_DEF = 2, 3


# ---------------------------------------------------------------- the definition
def _inputs(name):
    """Per-member detuned operators, u_scale != 1, a non-uniform grid, states that are not Hermitian."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(9700 + PLANTS.index(name))
    X = c.states(rng, B_DEF * T_DEF).reshape(B_DEF, T_DEF, c.n)
    X = X + 0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    d2 = c.d * c.d
    M = X.reshape(B_DEF, T_DEF, d2, -1) if c.kind == _lib.PLANT_PROCESS else X.reshape(B_DEF, T_DEF, c.d, c.d)
    assert np.abs(M - M.conj().swapaxes(-1, -2)).max() > 1e-2
    U = c.sat * rng.uniform(-1, 1, (B_DEF, T_DEF, c.m))
    sc = 1 + 0.1 * rng.standard_normal((B_DEF, c.m))
    op0, ops = c.member_ops(rng, B_DEF)
    ts = gc.grid(rng, T_DEF, c.dt)
    return c, rng, X, U, sc, op0, ops, ts


def _points(c, X, U, sc, op0, ops, ts):
    """(b, t, f) for every point: f(x, u) is the independent step of member b over interval t under the unscaled controls u."""
    dts = np.diff(ts)
    for b in range(X.shape[0]):
        for t in range(X.shape[1]):
            yield b, t, (lambda x, u, b=b, t=t: c.step(x, sc[b] * u, op0[b], list(ops[b]), dts[t]))


@pytest.mark.parametrize("name", PLANTS)
def test_definition_is_exact_at_the_point(name):
    """A x + B u + Delta against the independent step: test_grad_host.py's bound for its forward chain (measured 1.1e-16); and the
    columns of A against the step of the unit vectors - the step is linear in the state."""
    c, rng, X, U, sc, op0, ops, ts = _inputs(name)
    A, Bm, D = m4q.plant_linearize_reference(X, U, op0, ops, ts, c.kind, u_scale=sc)
    assert A.shape == (B_DEF, T_DEF, c.n, c.n) and Bm.shape == (B_DEF, T_DEF, c.n, c.m) and D.shape == (B_DEF, T_DEF, c.n)
    worst = worst_a = 0.0
    for b, t, f in _points(c, X, U, sc, op0, ops, ts):
        x, u = X[b, t], U[b, t]
        err = np.abs(A[b, t] @ x + Bm[b, t] @ u + D[b, t] - f(x, u)).max()
        worst = max(worst, err / max(1.0, np.abs(x).max()))
        assert err <= 1e-12 * max(1.0, np.abs(x).max())
        cols = np.stack([f(e, u) for e in np.identity(c.n, dtype=complex)], axis=1)
        worst_a = max(worst_a, np.abs(cols - A[b, t]).max())
        assert np.array_equal(D[b, t], -sum(Bm[b, t][:, k] * u[k] for k in range(c.m)))          # k ascending
    print("%s: A x + B u + Delta against the step %.2e, columns of A %.2e, max|B| = %.3e" % (name, worst, worst_a, np.abs(Bm).max()))
    assert worst_a <= 1e-12 and np.abs(Bm).max() > 1e-3


@pytest.mark.parametrize("name", PLANTS)
def test_B_against_central_differences(name):
    c, rng, X, U, sc, op0, ops, ts = _inputs(name)
    _, Bm, _ = m4q.plant_linearize_reference(X, U, op0, ops, ts, c.kind, u_scale=sc, outputs=("B",))
    worst = 0.0
    for b, t, f in _points(c, X, U, sc, op0, ops, ts):
        for k in range(c.m):
            e = np.zeros(c.m)
            e[k] = H_FD
            fd = (f(X[b, t], U[b, t] + e) - f(X[b, t], U[b, t] - e)) / (2 * H_FD)
            worst = max(worst, np.abs(fd - Bm[b, t][:, k]).max() / max(1.0, np.abs(Bm).max()))
    print("%s: B against central differences %.2e" % (name, worst))
    assert worst <= FD_BOUND


@pytest.mark.parametrize("name", PLANTS)
def test_remainder_is_of_second_order(name):
    """step(x + s dx, u + s du) - (A (x + s dx) + B (u + s du) + Delta) falls by 4 per halving of s (measured 3.98-4.01)."""
    c, rng, X, U, sc, op0, ops, ts = _inputs(name)
    A, Bm, D = m4q.plant_linearize_reference(X, U, op0, ops, ts, c.kind, u_scale=sc)
    for b, t, f in _points(c, X, U, sc, op0, ops, ts):
        du = 0.1 * c.sat * rng.standard_normal(c.m)
        dx = 0.1 * (rng.standard_normal(c.n) + 1j * rng.standard_normal(c.n))
        r = []
        for s in (1.0, 0.5, 0.25):
            x, u = X[b, t] + s * dx, U[b, t] + s * du
            r.append(np.abs(f(x, u) - (A[b, t] @ x + Bm[b, t] @ u + D[b, t])).max())
        print("%s b=%d t=%d: remainders %.2e %.2e %.2e, ratios %.3f %.3f" % (name, b, t, r[0], r[1], r[2], r[0] / r[1], r[1] / r[2]))
        assert r[2] > 1e-9                                     # (far above rounding: the ratios mean something)
        assert 3.5 <= r[0] / r[1] <= 4.5 and 3.5 <= r[1] / r[2] <= 4.5


def test_reference_layouts_and_optional_outputs():
    """Shared operators and controls, a scalar dt, no u_scale; an output not asked for is None and the others do not change."""
    c = gc.plant_case("9-2")
    rng = np.random.default_rng(9790)
    X = c.states(rng, 6).reshape(2, 3, c.n)
    U = c.sat * rng.uniform(-1, 1, (3, c.m))
    full = m4q.plant_linearize_reference(X, U, c.op0, c.ops, c.dt, c.kind)
    same = m4q.plant_linearize_reference(X, np.stack([U, U]), np.stack([c.op0] * 2), c.ops[None], np.arange(4) * c.dt, c.kind,
                                         u_scale=np.ones((2, c.m)))
    for a, b in zip(full, same):
        assert np.abs(a - b).max() <= 1e-14
    assert np.array_equal(full[0][0, 0], full[0][1, 0])        # A does not depend on the state
    for outputs in (("A",), ("Delta", "B"), ["B"]):
        got = m4q.plant_linearize_reference(X, U, c.op0, c.ops, c.dt, c.kind, outputs=outputs)
        for name, g, f in zip(plant_linearize.OUTPUTS, got, full):
            assert (g is None) if name not in outputs else np.array_equal(g, f)


# ---------------------------------------------------------------- the C ABI
def _buf(n):
    a = np.zeros(max(int(n), 1))
    return a, a.ctypes.data_as(DP)


class _LinCall:
    """One valid m4q_plant_linearize_batch call on host buffers of the right sizes; fields are replaced one at a time."""

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, T=4, k=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, kind=kind, T=T, dts=self._b("dts", T), X=self._b("X", 2 * B * T * n), U=self._b("U", T * m), u_per=0,
                      u_scale=None, op0=self._b("op0", 2 * k * k), ops=self._b("ops", 2 * m * k * k), per=0,
                      A=self._b("A", 2 * B * T * n * n), Bm=self._b("B", 2 * B * T * n * m), D=self._b("D", 2 * B * T * n))

    def _b(self, name, count):
        self.keep[name], p = _buf(count)
        return p

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_linearize_batch(v["B"], v["n"], v["m"], v["kind"], v["T"], v["dts"], v["X"], v["U"], v["u_per"],
                                                    v["u_scale"], v["op0"], v["ops"], v["per"], v["A"], v["Bm"], v["D"])


@pytest.mark.parametrize("change", [dict(B=0), dict(B=-2), dict(T=0), dict(T=-1), dict(dts=None), dict(X=None), dict(U=None), dict(op0=None),
                                    dict(ops=None), dict(A=None, Bm=None, D=None), dict(kind=0), dict(kind=4), dict(kind=-1),
                                    dict(kind=_lib.PLANT_PROCESS)], ids=str)
def test_c_abi_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _LinCall()(**change) == _lib.E_BADARG
    assert _lib.lib().m4q_last_error()


def test_c_abi_refuses_what_has_no_kernel():
    assert _LinCall(n=25, k=5)() == _lib.E_UNSUPPORTED                         # no compiled shape
    assert _LinCall(n=9, m=3)() == _lib.E_UNSUPPORTED
    assert _LinCall(n=8, m=2, k=2)() == _lib.E_UNSUPPORTED                     # a shape with a model and no device plant
    for call in (_LinCall(kind=_lib.PLANT_GENERATOR, k=9), _LinCall(n=16, m=3, kind=_lib.PLANT_GENERATOR, k=16)):
        assert call() == _lib.E_UNSUPPORTED
        msg = _lib.lib().m4q_last_error().decode()
        assert "m4q_discretize_batch" in msg and "m4q_linearize_batch" in msg


def test_valid_calls_need_a_device():
    """Every subset of the outputs, both plants, the plant-only shape, per-member everything: refused only for want of a device."""
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    for call in (_LinCall(), _LinCall(n=4, m=1, k=2), _LinCall(n=16, m=2, k=4), _LinCall(n=16, m=3, k=4),
                 _LinCall(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2), _LinCall(B=1, T=1)):
        assert call() == _lib.E_NODEVICE
        for gone in (dict(A=None), dict(Bm=None), dict(D=None), dict(A=None, Bm=None), dict(A=None, D=None), dict(Bm=None, D=None)):
            assert call(**gone) == _lib.E_NODEVICE
    c = gc.plant_case("4-1")
    with pytest.raises(_lib.M4qError):
        m4q.plant_linearize_batch(np.zeros((1, 2, 4)), np.zeros((2, 1)), c.op0, c.ops, c.dt)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library fails the test."""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)


def _good():
    c = gc.plant_case("9-2")
    B, T = 3, 4
    return c, dict(X=np.zeros((B, T, c.n), dtype=complex), U=np.zeros((B, T, c.m)), op0=c.op0, ops=c.ops, dt_or_ts=c.dt)


BAD_LIN = [
    (dict(X=np.zeros((4, 9))), ValueError), (dict(X=np.zeros((3, 4, 9, 1))), ValueError), (dict(X=np.zeros((0, 4, 9))), ValueError),
    (dict(X=np.zeros((3, 4, 8))), ValueError),                                    # n is not a square
    (dict(U=np.zeros((3, 4, 2), dtype=complex)), TypeError), (dict(U=np.zeros((3, 5, 2))), ValueError),
    (dict(U=np.zeros((2, 4, 2))), ValueError), (dict(U=np.zeros(4)), ValueError), (dict(U=np.zeros((3, 4, 3))), ValueError),
    (dict(u_scale=np.ones((3, 3))), ValueError), (dict(u_scale=np.ones(2)), ValueError),
    (dict(op0=np.eye(2)), ValueError), (dict(op0=np.zeros((2, 3, 3))), ValueError), (dict(ops=np.zeros((3, 3))), ValueError),
    (dict(ops=np.zeros((2, 2, 3, 3))), ValueError),
    (dict(dt_or_ts=np.zeros(4)), ValueError), (dict(dt_or_ts=np.zeros((5, 1))), ValueError), (dict(dt_or_ts=float("nan")), ValueError),
    (dict(kind=_lib.PLANT_GENERATOR), ValueError), (dict(kind=0), ValueError), (dict(kind=7), ValueError),
    (dict(kind=_lib.PLANT_PROCESS), ValueError),                                  # n = 9 is no fourth power
    (dict(outputs=()), ValueError), (dict(outputs=("A", "C")), ValueError), (dict(outputs="A"), TypeError), (dict(outputs=None), TypeError),
]


@pytest.mark.parametrize("change,error", BAD_LIN, ids=lambda v: str(v)[:60])
def test_plant_linearize_batch_refuses_before_the_library(no_library, change, error):
    c, good = _good()
    for fn in (m4q.plant_linearize_batch, m4q.plant_linearize_reference):
        with pytest.raises(error):
            fn(**dict(good, **change))


def test_experiment_wrappers_refuse_what_the_plant_cannot_do(no_library):
    c, good = _good()
    exp = m4q.QExperiment(c.op0, list(c.ops))
    exp.set("c_ops", [np.diag([0.0, 1.0, 0.0]).astype(complex)])
    with pytest.raises(ValueError, match="generator plant"):
        exp.linearize_batch(good["X"], good["U"], c.dt)
    with pytest.raises(ValueError, match="generator plant"):
        m4q.LExperiment(np.zeros((9, 9)), [np.zeros((9, 9))] * 2).linearize_batch(good["X"], good["U"], c.dt)
    with pytest.raises(ValueError):
        m4q.QSynthesis(c.op0, list(c.ops)).linearize_batch(good["X"], good["U"], c.dt)          # 9 is no fourth power
    with pytest.raises(ValueError):
        m4q.QExperiment(c.op0, list(c.ops)).linearize_batch(good["X"], good["U"][:, :3], c.dt)


def _good_law():
    c = gc.plant_case("9-2")
    N = 4
    return c, dict(op0=c.op0, ops=c.ops, dt_or_ts=c.dt, X_nom=np.zeros((N + 1, c.n), dtype=complex), U_nom=np.zeros((N, c.m)),
                   X_targ=np.zeros((N + 1, c.n), dtype=complex), U_targ=np.zeros((N, c.m)), Q_ls=np.eye(c.n), R_ls=np.eye(c.m), sat=1.0)


def _per(v, B=3):
    return dict(v, X_nom=np.zeros((B,) + v["X_nom"].shape, dtype=complex), U_nom=np.zeros((B,) + v["U_nom"].shape))


BAD_LAW = [
    (dict(X_nom=np.zeros(9)), ValueError), (dict(X_nom=np.zeros((3, 9))), ValueError), (dict(X_nom=np.zeros((7, 9))), ValueError),
    (dict(X_nom=np.zeros((3, 5, 9))), ValueError),                                # per-member states beside one control sequence
    (dict(U_nom=np.zeros((3, 4, 2))), ValueError), (dict(U_nom=np.zeros((4, 2), dtype=complex)), TypeError),
    (dict(U_nom=np.zeros((0, 2)), X_nom=np.zeros((1, 9))), ValueError),
    (dict(X_targ=np.zeros((4, 9))), ValueError), (dict(X_targ=np.zeros((3, 5, 9))), ValueError),       # a leading B beside one nominal
    (dict(U_targ=np.zeros((5, 2))), ValueError), (dict(U_targ=np.zeros((4, 2), dtype=complex)), TypeError),
    (dict(Q_ls=np.eye(4)), ValueError), (dict(Q_ls=np.zeros((4, 9, 9))), ValueError), (dict(R_ls=np.eye(3)), ValueError),
    (dict(R_ls=np.zeros((5, 2, 2))), ValueError),
    (dict(sat=0.0), ValueError), (dict(sat=-1.0), ValueError), (dict(du=0.0, u_prev=np.zeros(2)), ValueError), (dict(du=0.5), ValueError),
    (dict(du=0.5, u_prev=np.zeros(3)), ValueError), (dict(du=0.5, u_prev=np.zeros((3, 2))), ValueError),  # one nominal: one QP
    (dict(u_scale=np.ones((2, 2))), ValueError), (dict(u_scale=np.ones(2)), ValueError),
    (dict(op0=np.eye(2)), ValueError), (dict(ops=np.zeros((3, 3, 3))), ValueError), (dict(dt_or_ts=np.zeros(4)), ValueError),
    (dict(kind=_lib.PLANT_GENERATOR), ValueError), (dict(kind=_lib.PLANT_PROCESS), ValueError), (dict(kind=9), ValueError),
]
BAD_LAW_PER = [
    (dict(U_nom=np.zeros((2, 4, 2))), ValueError), (dict(X_targ=np.zeros((2, 5, 9))), ValueError), (dict(U_targ=np.zeros((2, 4, 2))), ValueError),
    (dict(du=0.5, u_prev=np.zeros((2, 2))), ValueError), (dict(u_scale=np.ones((2, 2))), ValueError), (dict(op0=np.zeros((2, 3, 3))), ValueError),
    (dict(ops=np.zeros((2, 2, 3, 3))), ValueError), (dict(dt_or_ts=np.zeros(6)), ValueError),
]


@pytest.mark.parametrize("change,error", BAD_LAW, ids=lambda v: str(v)[:60])
def test_along_plant_trajectory_refuses_before_the_library(no_library, change, error):
    c, good = _good_law()
    with pytest.raises(error):
        m4q.FeedbackLaw.along_plant_trajectory(**dict(good, **change))


@pytest.mark.parametrize("change,error", BAD_LAW_PER, ids=lambda v: str(v)[:60])
def test_per_member_along_plant_trajectory_refuses_before_the_library(no_library, change, error):
    c, good = _good_law()
    with pytest.raises(error):
        m4q.FeedbackLaw.along_plant_trajectory(**dict(_per(good), **change))


def test_along_trajectory_is_as_it_was():
    """The model-side constructor keeps its signature: the plant-side twin is a new name beside it."""
    import inspect
    assert list(inspect.signature(m4q.FeedbackLaw.along_trajectory).parameters) == [
        "model", "order", "X_nom", "U_nom", "X_targ", "U_targ", "Q_ls", "R_ls", "sat", "du", "u_prev", "exact"]
    assert list(inspect.signature(m4q.FeedbackLaw.along_plant_trajectory).parameters) == [
        "op0", "ops", "dt_or_ts", "X_nom", "U_nom", "X_targ", "U_targ", "Q_ls", "R_ls", "sat", "du", "u_prev", "kind", "u_scale", "exact"]

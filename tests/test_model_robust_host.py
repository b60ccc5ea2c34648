"""The robust optimiser on models (m4q_model_robust_batch) and its multi rollout (m4q_model_rollout_multi_batch) without a GPU: the
NumPy definitions of mpc4quantum_amd/model_robust.py - the multi rollout against the independent model chain, the loop against
plant_robust_reference on the same callables, the decisions under a gradient pushed by its bound on every model shape, a
dissipative qubit end to end against the generator plant's own expm - the prototypes, every refusal of the two C entries before a
device is asked for and every ValueError of the wrappers before the library is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd import model_robust as mr
from mpc4quantum_amd import plant_robust as pr
from tests import grad_cases as gc
from tests import model_robust_cases as mc
from tests import plant_robust_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP = _lib._dp, _lib._ip


# ---------------------------------------------------------------- the multi reference
@pytest.mark.parametrize("per_member", [True, False], ids=["per-member", "shared"])
@pytest.mark.parametrize("shape", [(4, 1, 2), (8, 2, 1)], ids=str)
def test_multi_reference_is_the_figure_of_the_independent_chain(shape, per_member):
    n, m, order = shape
    B, N, S = 3, 4, 3
    k = mc.case(shape, B, N, 5100 + n)
    x0, U0, models, _, W, f, sat = k["args"]
    sc, w = k["kw"]["u_scale"], k["kw"]["weights"]
    if not per_member:
        models = models[1]
    us = np.stack([U0, 0.5 * U0, -U0])
    for figure in ("last", "sum"):
        for scale in (sc, None):
            out = m4q.model_rollout_multi_reference(x0, us, models, order, W, f, u_scale=scale, figure=figure, weights=w)
            assert out["J"].shape == (B, S) and out["F"].shape == (S,)
            for b in range(B):
                for s in range(S):
                    v = us[s] * (1.0 if scale is None else scale[b][None, :])
                    q = gc.figures(gc.model_chain(models[b] if per_member else models, m, order, x0[b], v), W, f[b])
                    want = q[-1] if figure == "last" else q.sum()
                    assert abs(out["J"][b, s] - want) <= 1e-12 * max(1.0, abs(want)), (b, s)
            assert np.array_equal(out["F"], m4q.ordered_weighted_sum(out["J"], w))
            for s in range(S):           # ... and the reduced gradient's own objective, bit for bit
                ref = m4q.model_rollout_grad_reference(x0, us[s], models, order, W, f, u_scale=scale, figure=figure, weights=w, reduce=True)
                assert ref["q_mean"] == out["F"][s]
    only_F = m4q.model_rollout_multi_reference(x0, us, models, order, W, f, members=False)
    only_J = m4q.model_rollout_multi_reference(x0, us[0], models, order, W, f, mean=False)
    assert set(only_F) == {"F"} and set(only_J) == {"J"} and only_J["J"].shape == (B, 1)


# ---------------------------------------------------------------- the loop
@pytest.mark.parametrize("mem", [0, 3])
def test_model_robust_reference_is_the_plant_loop_on_the_same_callables(mem):
    k = mc.case((4, 1, 2), 5, 5, 5200)
    kw = dict(iters=4, steps=4, mem=mem, step0=rc.STEP0, tol=0.0)
    mine = m4q.model_robust_reference(*k["args"], figure="sum", members=True, **k["kw"], **kw)
    theirs = m4q.plant_robust_reference(None, k["args"][1], None, None, None, None, None, k["args"][6], members=True,
                                        evaluate=mc.reference_evaluate(k, "sum"), **kw)
    assert set(mine) == set(theirs)
    for key in mine:
        assert np.array_equal(mine[key], theirs[key]), key
    assert np.count_nonzero(mine["alpha_hist"]) >= 2 and mine["cost"] < mine["cost_hist"][0]
    assert float(m4q.ordered_weighted_sum(mine["J"], k["kw"]["weights"])) == mine["cost"]
    # evaluate= drives model_robust_reference as it drives the plant's
    again = m4q.model_robust_reference(None, k["args"][1], None, None, None, None, k["args"][6], evaluate=mc.reference_evaluate(k, "sum"), **kw)
    assert np.array_equal(again["U"], mine["U"]) and again["cost"] == mine["cost"]


@pytest.mark.parametrize("mem", mc.MEMS)
@pytest.mark.parametrize("figure", mc.FIGURES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_a_gradient_pushed_by_its_bound_changes_no_decision(shape, figure, mem):
    """The cells of the device's comparison with the NumPy definition (tests/test_gpu_model_robust.py): on them the definition takes
    the same decisions when every gradient is pushed by the project's gradient bound, and what moves is of the order of the push."""
    plain, pushed = mc.definition_runs(shape, figure, mem)
    assert np.array_equal(plain["alpha_hist"], pushed["alpha_hist"])
    assert (plain["status"], plain["n_iter"]) == (pushed["status"], pushed["n_iter"])
    dU, dF = rc.movement(plain, pushed)
    print("%s %s mem %d: status %d, alpha %s; the pushed run moved U by %.2e and cost_hist by %.2e"
          % (shape, figure, mem, plain["status"], plain["alpha_hist"], dU, dF))
    assert 0 < dU <= 1e-6 and 0 < dF <= 1e-6


def test_the_cells_hold_a_rejected_step_with_memory_and_a_converged_run():
    plain, _ = mc.definition_runs((8, 2, 1), "last", 3)              # rejected with memory: the memory is cleared, the run goes on
    assert plain["status"] == pr.STATUS_ITERS and np.array_equal(plain["alpha_hist"] > 0, [True, False, True])
    # (16, 1, 4), "sum", mem 3 under the cells' common seed: status 1 with every entry of U on the box, the same under the pushed
    # gradient - and so a movement of exactly 0 in U, which is why the cell of the bound has a seed of its own
    seed = 9400 + 11 * mc.SHAPES.index((16, 1, 4))
    assert mc.seed_of((16, 1, 4), "sum", 3) != seed and mc.seed_of((16, 1, 4), "sum", 0) == seed
    plain, pushed = mc.definition_runs((16, 1, 4), "sum", 3, seed=seed)
    assert (plain["status"], plain["n_iter"]) == (pushed["status"], pushed["n_iter"]) == (pr.STATUS_CONVERGED, 3)
    assert np.array_equal(plain["alpha_hist"], pushed["alpha_hist"]) and np.array_equal(plain["alpha_hist"] > 0, [True, True, False])
    sat = mc.parity_case((16, 1, 4), "sum", 3, seed)["args"][6]
    assert np.all(np.abs(plain["U"]) == sat) and plain["pgrad_hist"][2] == 0 and rc.movement(plain, pushed)[0] == 0


def test_statuses_of_the_definition():
    args, kw = mc.own_trajectory_case()
    out = m4q.model_robust_reference(*args, **kw)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NO_DESCENT, 1) and 0 < out["cost"] < 1e-15
    assert np.array_equal(out["U"], args[1]) and np.all(out["alpha_hist"] == 0)
    bad = args[0].copy()
    bad[0, 1] = np.nan
    out = m4q.model_robust_reference(bad, *args[1:], **kw)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NOT_FINITE, 0) and np.isnan(out["cost"])


# ---------------------------------------------------------------- dissipative dynamics, end to end
def test_a_pulse_optimised_on_the_models_lowers_the_generator_plants_own_mean():
    """Optimised on the order-2 models of the members' Lindblad generators; judged on the generator plant itself (SciPy's expm)."""
    c, d = mc.dissipative_case(), mc.DISSIPATIVE
    gens = [c["L0"], np.broadcast_to(c["L1"], c["L0"].shape)]
    results = {}
    for order in (2, 1):
        models = m4q.discretize_homogeneous(gens, d["dt"], order)
        out = m4q.model_robust_reference(c["x0"], c["U0"], models, order, c["W"], c["target"], d["sat"], u_scale=c["u_scale"], figure="last",
                                         iters=d["iters"], steps=d["steps"], mem=d["mem"], step0=d["step0"], tol=d["tol"])
        results[order] = (out, mc.generator_plant_mean(c, out["U"]))
    before = mc.generator_plant_mean(c, c["U0"])
    out, after = results[2]
    print("order 2: the model mean goes %.3f -> %.3f, the generator plant's %.3f -> %.3f (order 1: %.3f)"
          % (out["cost_hist"][0], out["cost"], before, after, results[1][1]))
    assert after < before
    assert np.all(np.diff(out["cost_hist"]) <= 0) and out["cost"] < out["cost_hist"][0]
    assert np.all(np.abs(out["U"]) <= d["sat"])


# ---------------------------------------------------------------- prototypes and exports
@pytest.mark.parametrize("symbol,count", [("m4q_model_rollout_multi_batch", 18), ("m4q_model_robust_batch", 30)])
def test_header_and_prototype_table_agree(symbol, count):
    header = open(os.path.join(ROOT, "include", "m4q.h")).read()
    decl = re.search(r"M4Q_API int %s\((.*?)\);" % symbol, header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "const double*": DP, "double*": DP, "int32_t*": IP}
    mine = [ctype[p.rsplit(" ", 1)[0]] for p in params]
    restype, argtypes = _lib.PROTOTYPES[symbol]
    assert restype is ctypes.c_int and argtypes == mine and len(mine) == count
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol)


def test_exports():
    for name in ("model_rollout_multi_batch", "model_rollout_multi_reference", "model_robust_batch", "model_robust_reference"):
        assert getattr(m4q, name) is getattr(mr, name)
    for cls in (m4q.QExperiment, m4q.LExperiment):
        assert callable(cls.robust_model_batch)
    assert m4q.LExperiment.robust_model_batch is m4q.QExperiment.robust_model_batch
    assert not hasattr(m4q.QSynthesis, "robust_model_batch")


# ---------------------------------------------------------------- the C entry points
def _buf(n, dtype=np.float64):
    a = np.zeros(max(int(n), 1), dtype=dtype)
    return a, a.ctypes.data_as(IP if dtype == np.int32 else DP)


class _Call:
    def _b(self, name, count, dtype=np.float64):
        self.keep[name], p = _buf(count, dtype)
        return p

    def weights(self, values):
        self.keep["w"] = np.array(values, dtype=np.float64)
        return self.keep["w"].ctypes.data_as(DP)

    def __call__(self, **change):
        v = dict(self.v, **change)
        return getattr(_lib.lib(), self.SYMBOL)(*[v[k] for k in self.ORDER])


class _MultiCall(_Call):
    """One valid m4q_model_rollout_multi_batch call on host buffers of the right sizes; fields are replaced one at a time."""
    SYMBOL = "m4q_model_rollout_multi_batch"
    ORDER = ("B", "n", "m", "order", "N", "x0", "S", "us", "u_scale", "models", "per", "W", "target", "t_per", "q_mode", "weights", "J", "F")

    def __init__(self, B=3, n=9, m=2, order=1, N=4, P=2, S=3):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, order=order, N=N, x0=self._b("x0", 2 * B * n), S=S, us=self._b("us", 8 * N * m), u_scale=None,
                      models=self._b("models", 2 * n * n * (1 + P)), per=0, W=self._b("W", 2 * n * n), target=self._b("f", 2 * n), t_per=0,
                      q_mode=2, weights=None, J=self._b("J", 8 * B), F=self._b("F", 8))


class _RobustCall(_Call):
    """... and one valid m4q_model_robust_batch call."""
    SYMBOL = "m4q_model_robust_batch"
    ORDER = ("B", "n", "m", "order", "N", "x0", "U0", "u_scale", "models", "per", "W", "target", "t_per", "q_mode", "weights", "sat", "iters",
             "steps", "mem", "step0", "tol", "gtol", "U", "cost", "cost_hist", "alpha_hist", "pgrad_hist", "n_iter", "status", "J")

    def __init__(self, B=3, n=9, m=2, order=1, N=4, P=2):
        self.keep = {}
        self.v = dict(B=B, n=n, m=m, order=order, N=N, x0=self._b("x0", 2 * B * n), U0=self._b("U0", N * m), u_scale=None,
                      models=self._b("models", 2 * n * n * (1 + P)), per=0, W=self._b("W", 2 * n * n), target=self._b("f", 2 * n), t_per=0,
                      q_mode=1, weights=None, sat=1.0, iters=2, steps=3, mem=2, step0=0.1, tol=1e-9, gtol=0.0, U=self._b("U", N * m),
                      cost=self._b("cost", 1), cost_hist=self._b("ch", 65), alpha_hist=self._b("ah", 64), pgrad_hist=self._b("ph", 64),
                      n_iter=self._b("ni", 1, np.int32), status=self._b("st", 1, np.int32), J=self._b("J", B))


SHARED_BAD = [dict(B=0), dict(B=-2), dict(N=0), dict(N=-1), dict(x0=None), dict(W=None), dict(target=None), dict(q_mode=0),
              dict(q_mode=3), dict(q_mode=-1), dict(models=None)]
MULTI_BAD = SHARED_BAD + [dict(us=None), dict(S=0), dict(S=9), dict(S=-1), dict(J=None, F=None)]
ROBUST_BAD = SHARED_BAD + [dict(U0=None), dict(U=None), dict(cost=None), dict(cost_hist=None), dict(alpha_hist=None), dict(pgrad_hist=None),
                           dict(n_iter=None), dict(status=None), dict(sat=0.0), dict(sat=-1.0), dict(sat=np.nan), dict(iters=0),
                           dict(iters=65), dict(steps=0), dict(steps=9), dict(mem=-1), dict(mem=9), dict(step0=0.0), dict(step0=-0.1),
                           dict(step0=np.inf), dict(step0=np.nan), dict(tol=-1e-9), dict(tol=np.inf), dict(tol=np.nan),
                           dict(gtol=-1e-9), dict(gtol=np.inf), dict(gtol=np.nan)]
BAD_WEIGHTS = [[1.0, np.nan, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -1e-300], [-1.0, 1.0, 1.0]]


@pytest.mark.parametrize("change", MULTI_BAD, ids=str)
def test_multi_rollout_refuses_bad_arguments(change):
    assert _MultiCall()(**change) == _lib.E_BADARG
    assert b"m4q_model_rollout_multi_batch" in _lib.lib().m4q_last_error()


@pytest.mark.parametrize("change", ROBUST_BAD, ids=str)
def test_robust_refuses_bad_arguments(change):
    assert _RobustCall()(**change) == _lib.E_BADARG
    assert b"m4q_model_robust_batch" in _lib.lib().m4q_last_error()


@pytest.mark.parametrize("values", BAD_WEIGHTS, ids=str)
def test_both_refuse_bad_weights(values):
    for call in (_MultiCall(), _RobustCall()):
        assert call(weights=call.weights(values)) == _lib.E_BADARG
    m = _MultiCall()
    assert m(weights=m.weights(values), F=None) == _lib.E_BADARG     # (checked even where no mean is asked for)


@pytest.mark.parametrize("Call", [_MultiCall, _RobustCall])
def test_both_refuse_what_has_no_model_kernel(Call):
    for change in (dict(n=25), dict(n=9, m=3), dict(n=9, m=2, order=3), dict(n=16, m=2, order=1), dict(order=0)):
        assert Call(**change)() == _lib.E_UNSUPPORTED, change       # (16, 2, 1) is a plant-only shape: no model kernel
        err = _lib.lib().m4q_last_error()
        assert Call.SYMBOL.encode() in err and b"no model kernel" in err
    assert Call(n=25)(B=0) == _lib.E_UNSUPPORTED                    # (the shape is looked up first)


def test_well_formed_calls_reach_the_device():
    """Every check passed: the call asks for a device (and, where there is one, runs on the all-zero data)."""
    want = 0 if _lib.device_count() > 0 else _lib.E_NODEVICE
    assert _MultiCall()() == want
    assert _MultiCall()(S=1, q_mode=1, F=None) == want and _MultiCall()(S=8, J=None) == want
    m = _MultiCall()
    assert m(weights=m.weights([0.0, 1.0, 2.5])) == want
    assert _MultiCall(n=8, m=2, order=1, P=2)() == want                        # a shape with a model and no device plant
    assert _MultiCall(n=16, m=1, order=4, P=4)() == want
    assert _RobustCall()() == want
    assert _RobustCall()(J=None, q_mode=2, mem=0, iters=64, steps=8, sat=np.inf) == want
    assert _RobustCall(n=9, m=2, order=2, P=5)() == want
    assert _RobustCall(n=4, m=1, order=1, P=1)() == want


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, n=9, m=2, order=1, P=2, **more):
    return dict(more, x0=np.zeros((B, n), complex), models=np.zeros((n, n * (1 + P)), complex), order=order, W=np.eye(n), target=np.zeros(n))


SHAPES_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((0, 9))), dict(u_scale=np.ones((3, 1))), dict(u_scale=np.ones(2)), dict(W=None),
              dict(target=None), dict(W=np.eye(4)), dict(target=np.zeros(4)), dict(target=np.zeros((2, 9))), dict(figure="all"),
              dict(figure="none"), dict(weights=np.ones(2)), dict(weights=[1.0, np.nan, 1.0]), dict(weights=[1.0, -1.0, 1.0]),
              dict(models=np.zeros((9, 9))), dict(models=np.zeros((2, 9, 27))), dict(models=np.zeros((9, 27, 1, 1))), dict(order=0),
              dict(order=2)]


def _ident(c):
    return ",".join("%s%s" % (k, getattr(v, "shape", v)) for k, v in c.items())


@pytest.mark.parametrize("change", SHAPES_BAD + [dict(us=np.zeros(4)), dict(us=np.zeros((9, 4, 2))), dict(us=np.zeros((2, 3, 4, 2))),
                                                 dict(us=np.zeros((0, 4, 2))), dict(members=False, mean=False)], ids=_ident)
def test_multi_wrapper_refuses_bad_arguments(no_library, change):
    for fn in (m4q.model_rollout_multi_batch, m4q.model_rollout_multi_reference):
        with pytest.raises(ValueError):
            fn(**dict(_args(us=np.zeros((3, 4, 2))), **change))


@pytest.mark.parametrize("change", SHAPES_BAD + [dict(U0=np.zeros(4)), dict(U0=np.zeros((3, 4, 2))), dict(sat=0.0), dict(sat=np.nan),
                                                 dict(iters=0), dict(iters=65), dict(steps=0), dict(steps=9), dict(mem=-1), dict(mem=9),
                                                 dict(step0=0.0), dict(step0=np.inf), dict(tol=-1.0), dict(tol=np.nan), dict(gtol=-1.0),
                                                 dict(gtol=np.inf)], ids=_ident)
def test_robust_wrapper_refuses_bad_arguments(no_library, change):
    for fn in (m4q.model_robust_batch, m4q.model_robust_reference):
        with pytest.raises(ValueError):
            fn(**dict(_args(U0=np.zeros((4, 2)), sat=1.0), **change))


def test_integer_parameters_must_be_integers(no_library):
    for change in (dict(iters=2.5), dict(steps=True), dict(mem=1.5)):
        with pytest.raises(TypeError):
            m4q.model_robust_batch(**dict(_args(U0=np.zeros((4, 2)), sat=1.0), **change))


def test_experiment_wrapper_refuses_before_the_library(no_library):
    x0 = np.zeros((3, 9), complex)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    ok = dict(x0=x0, U0=np.zeros((4, 2)), dt=0.25, order=1, W=np.eye(9), target=np.zeros(9), sat=1.0)
    with pytest.raises(ValueError, match="own step"):
        exp.robust_model_batch(**dict(ok, dt=np.linspace(0, 1, 5)))                      # a time grid
    for change in (dict(U0=np.zeros((4, 3))), dict(mem=9), dict(dt=0.0), dict(dt=np.inf), dict(order=0), dict(order=5), dict(order=1.5),
                   dict(x0=np.zeros((3, 4), complex), W=np.eye(4), target=np.zeros(4)), dict(op0=np.zeros((2, 3, 3))),
                   dict(op0=np.zeros((3, 9, 9))), dict(figure="all"), dict(weights=np.ones(2))):
        with pytest.raises(ValueError):
            exp.robust_model_batch(**dict(ok, **change))
    lexp = m4q.LExperiment(np.eye(9), [np.eye(9)] * 2)
    with pytest.raises(ValueError, match="own step"):
        lexp.robust_model_batch(**dict(ok, dt=[0.0, 0.5, 1.0, 1.5, 2.0]))
    with pytest.raises(ValueError):
        lexp.robust_model_batch(**dict(ok, op0=np.zeros((3, 3, 3))))                     # an LExperiment's op0 are generators
    # the refusals of robust_batch stay as they were
    with pytest.raises(ValueError, match="model_rollout_grad_batch"):
        lexp.robust_batch(x0, np.zeros((4, 2)), 0.25, np.eye(9), np.zeros(9), 1.0)


def test_robust_batch_still_refuses_collapse_operators():
    """(By the C entry, before a device is asked for: the generator plant has no gradient kernel.)"""
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    exp.set("c_ops", [np.eye(3)])
    with pytest.raises(_lib.M4qError, match="m4q_model_rollout_grad_batch"):
        exp.robust_batch(np.zeros((3, 9), complex), np.zeros((4, 2)), 0.25, np.eye(9), np.zeros(9), 1.0)


@pytest.mark.parametrize("route", ["hamiltonian-per-member", "hamiltonian-shared", "collapse-shared", "generators-per-member-order-3"])
def test_robust_model_batch_hands_down_the_models_of_the_right_generators(monkeypatch, route):
    """Every branch of robust_model_batch without a device: liouvillian(H) of a Hamiltonian plant, the generators as they stand with
    collapse operators and on an LExperiment, per-member op0 in that form or one shared model, the host discretisation at order 3.
    (The device discretisation is stood in for by the host's, which it is pinned to elsewhere.)"""
    from mpc4quantum_amd import vectorize
    from mpc4quantum_amd.configs import SX, SZ
    seen = {}

    class Fake:
        def m4q_model_robust_batch(self, *a):
            seen["robust"] = a
            return 0

        def m4q_last_error(self):
            return b""

    def on_host(gens, dt, order, scales=None):
        seen["device_discretise"] = order
        per = any(np.ndim(g) == 3 for g in gens)
        Bn = max(np.shape(g)[0] for g in gens if np.ndim(g) == 3) if per else 1
        return m4q.discretize_homogeneous([np.broadcast_to(g, (Bn,) + np.shape(g)[-2:]) for g in gens], dt, order)
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    monkeypatch.setattr(vectorize, "discretize_homogeneous_batch", on_host)
    B, N, n, dt = 3, 4, 4, 0.25
    H0, H1 = 0.15 * SZ, 0.5 * SX
    xi = np.array([0.9, 1.0, 1.1])
    order, op0 = 2, None
    if route.startswith("hamiltonian"):
        exp = m4q.QExperiment(H0, [H1])
        if route.endswith("per-member"):
            op0 = xi[:, None, None] * H0
            want = m4q.discretize_homogeneous([m4q.liouvillian(op0), np.broadcast_to(m4q.liouvillian(H1), (B, n, n))], dt, order)
        else:
            want = m4q.discretize_homogeneous([m4q.liouvillian(H0), m4q.liouvillian(H1)], dt, order)
    elif route == "collapse-shared":
        exp = m4q.QExperiment(H0, [H1])
        exp.set("c_ops", [np.sqrt(0.02) * SZ])
        L0, Lk = exp.operators()
        assert np.abs(L0 - m4q.liouvillian(H0)).max() > 1e-3
        want = m4q.discretize_homogeneous([L0, Lk[0]], dt, order)
    else:
        order = 3
        L0, L1 = m4q.liouvillian(H0), m4q.liouvillian(H1)
        exp = m4q.LExperiment(L0, [L1])
        op0 = xi[:, None, None] * L0
        want = m4q.discretize_homogeneous([op0, np.broadcast_to(L1, (B, n, n))], dt, order)
    out = exp.robust_model_batch(np.zeros((B, n), complex), np.zeros((N, 1)), dt, order, np.eye(n), np.zeros(n), 1.0, op0=op0, iters=2)
    a = seen["robust"]
    per = op0 is not None
    assert a[:5] == (B, n, 1, order, N) and a[9] == (1 if per else 0) and a[16] == 2
    assert want.shape == ((B, n, want.shape[-1]) if per else (n, want.shape[-1]))
    got = np.ctypeslib.as_array(a[8], want.shape[:-1] + (2 * want.shape[-1],)).view(complex)
    assert np.array_equal(got, want) and np.array_equal(out["models"], want)
    assert seen.get("device_discretise") == (order if order <= 2 else None)


def test_wrappers_hand_the_library_what_they_were_given(monkeypatch):
    seen = {}

    class Fake:
        def m4q_model_rollout_multi_batch(self, *a):
            seen["multi"] = a
            return 0

        def m4q_model_robust_batch(self, *a):
            seen["robust"] = a
            return 0

        def m4q_last_error(self):
            return b""
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    B, n, m, N = 3, 9, 2, 4
    us = np.arange(2 * N * m, dtype=float).reshape(2, N, m)
    models = np.arange(B * n * 3 * n, dtype=complex).reshape(B, n, 3 * n)
    out = m4q.model_rollout_multi_batch(np.zeros((B, n)), us, models, 1, np.eye(n), np.zeros((B, n)), u_scale=np.ones((B, m)), figure="sum",
                                        weights=[1.0, 2.0, 3.0])
    a = seen["multi"]
    assert len(a) == 18 and a[:5] == (B, n, m, 1, N) and a[6] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[7], (2, N, m)), us) and a[8] is not None and a[10] == 1 and a[13] == 1 and a[14] == 2
    assert np.array_equal(np.ctypeslib.as_array(a[9], (B, n, 6 * n)).view(complex), models)
    assert np.array_equal(np.ctypeslib.as_array(a[15], (B,)), [1.0, 2.0, 3.0])
    assert out["J"].shape == (B, 2) and out["F"].shape == (2,)
    out = m4q.model_rollout_multi_batch(np.zeros((B, n)), us[0], models[0], 1, np.eye(n), np.zeros(n), members=False)
    a = seen["multi"]
    assert a[6] == 1 and a[8] is None and a[10] == 0 and a[13] == 0 and a[14] == 1 and a[15] is None and a[16] is None
    assert set(out) == {"F"} and out["F"].shape == (1,)
    out = m4q.model_robust_batch(np.zeros((B, n)), us[1], models, 1, np.eye(n), np.zeros(n), np.inf, figure="sum", iters=7, steps=5, mem=0,
                                 step0=0.25, tol=1e-7, gtol=1e-3, members=True)
    a = seen["robust"]
    assert len(a) == 30 and a[:5] == (B, n, m, 1, N)
    assert np.array_equal(np.ctypeslib.as_array(a[6], (N, m)), us[1]) and a[7] is None and a[9] == 1 and a[12] == 0 and a[13] == 2
    assert a[14] is None and a[15:22] == (np.inf, 7, 5, 0, 0.25, 1e-7, 1e-3) and a[29] is not None
    assert out["U"].shape == (N, m) and out["cost_hist"].shape == (8,) and out["alpha_hist"].shape == (7,)
    assert out["pgrad_hist"].shape == (7,) and out["J"].shape == (B,) and isinstance(out["cost"], float)
    out = m4q.model_robust_batch(np.zeros((B, n)), us[1], models[:1], 1, np.eye(n), np.zeros(n), 1.0)
    assert seen["robust"][29] is None and seen["robust"][9] == 0 and "J" not in out

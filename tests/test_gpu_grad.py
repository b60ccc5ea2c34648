"""The rollout gradients on the device (plant_rollout_grad_kernel, model_rollout_grad_kernel, grad_reduce_kernel) against the
NumPy / SciPy definitions of mpc4quantum_amd/grad.py, which tests/test_grad_host.py holds to central differences.  Tolerance of
DESIGN section 3: 1e-10 max(1, max|g_ref|).  Shapes are the smallest that can go wrong: B = 5 (a ragged quad) and B = 1, N in {1, 6};
B = 1,030 for the reduction (five chunks, the last ragged); one case with 4,098 quads, past the grid the launch is capped at."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from tests import grad_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-10

# what is shared by the ensemble and what is the member's own
#   shared  one operator set, one control sequence, u_scale, a non-uniform grid, per-member targets
#   per     per-member operators and control sequences, no u_scale, a scalar dt, one target
RUNS = [("shared", 5, 6), ("per", 5, 6), ("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]
PLANTS = gc.PLANT_NAMES + ("16-2",)                                # the six cases and the plant-only shape


def _compare(out, ref, what):
    for key in ("grad", "grad_scale"):
        err = np.abs(out[key] - ref[key]).max() / max(1.0, np.abs(ref[key]).max())
        print("%s %s: max|g_ref| = %.3e, max|dg| / max(1, max|g_ref|) = %.2e" % (what, key, np.abs(ref[key]).max(), err))
        assert out[key].shape == ref[key].shape and np.isfinite(out[key]).all()
        assert err <= TOL
    assert np.abs(ref["grad"]).max() > 1e-3


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("variant,B,N", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", PLANTS)
def test_plant_gradient_against_the_reference(name, variant, B, N, figure):
    c = gc.plant_case(name)
    rng = np.random.default_rng(9500 + 13 * PLANTS.index(name) + 101 * B + N + (1000 if figure == "sum" else 0))
    x0 = c.states(rng, B)
    W, f = gc.weights_and_targets(rng, c.n, B)
    if variant == "per":
        op0, ops = c.member_ops(rng, B)
        u, ts, sc, f = rng.uniform(-c.sat, c.sat, (B, N, c.m)), c.dt, None, f[0]
    else:
        op0, ops = c.op0, c.ops
        u, ts, sc = rng.uniform(-c.sat, c.sat, (N, c.m)), gc.grid(rng, N, c.dt), 1 + 0.1 * rng.standard_normal((B, c.m))
    ref = m4q.plant_rollout_grad_reference(x0, u, op0, ops, ts, W, f, c.kind, u_scale=sc, figure=figure)
    out = m4q.plant_rollout_grad_batch(x0, u, op0, ops, ts, W, f, c.kind, u_scale=sc, figure=figure, scale_grad=True)
    assert set(out) == {"q", "grad", "grad_scale"}
    _compare(out, ref, "%s %s B=%d N=%d %s" % (name, variant, B, N, figure))
    # the forward pass is the rollout's own: the same figure, bit for bit
    roll = m4q.plant_rollout_batch(x0, u, op0, ops, ts, c.kind, u_scale=sc, W=W, target=f, keep="none",
                                   figure="last" if figure == "last" else "all")
    assert np.array_equal(out["q"], roll["q"])
    # without grad_scale the gradient is the same
    plain = m4q.plant_rollout_grad_batch(x0, u, op0, ops, ts, W, f, c.kind, u_scale=sc, figure=figure)
    assert set(plain) == {"q", "grad"} and np.array_equal(plain["grad"], out["grad"]) and np.array_equal(plain["q"], out["q"])


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("variant,B,N", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", gc.MODEL_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_model_gradient_against_the_reference(shape, variant, B, N, figure):
    n, m, order = shape
    models, x0, sat, rng = gc.model_case(n, m, order, B, 9600 + 100 * n + 10 * m + order + 7 * B + N + (1000 if figure == "sum" else 0))
    W, f = gc.weights_and_targets(rng, n, B)
    if variant == "per":
        u, sc, f = rng.uniform(-sat, sat, (B, N, m)), None, f[0]
    else:
        models = models[0]
        u, sc = rng.uniform(-sat, sat, (N, m)), 1 + 0.1 * rng.standard_normal((B, m))
    ref = m4q.model_rollout_grad_reference(x0, u, models, order, W, f, u_scale=sc, figure=figure)
    out = m4q.model_rollout_grad_batch(x0, u, models, order, W, f, u_scale=sc, figure=figure, scale_grad=True)
    _compare(out, ref, "model (%d, %d, %d) %s B=%d N=%d %s" % (n, m, order, variant, B, N, figure))
    roll = m4q.model_rollout_batch(x0, u, models, order, u_scale=sc, W=W, target=f, keep="none", figure="last" if figure == "last" else "all")
    assert np.array_equal(out["q"], roll["q"])


# ---------------------------------------------------------------- the ensemble reduction
def _objectives(q):
    """A member's objective from its figures, t ascending (grad.py)."""
    if q.ndim == 1:
        return 0.0 + q
    J = np.zeros(q.shape[0])
    for t in range(q.shape[1]):
        J = J + q[:, t]
    return J


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weights"])
@pytest.mark.parametrize("what", ["plant", "model"])
def test_reduction_is_the_ordered_sum_of_the_members(what, weighted, figure):
    B, N = 1030, 3
    c = gc.plant_case("4-1")
    rng = np.random.default_rng(9700 + (1 if weighted else 0) + (2 if figure == "sum" else 0))
    x0 = np.tile(c.states(rng, 32), (B // 32 + 1, 1))[:B] * (1 + 1e-3 * rng.standard_normal((B, 1)))
    u = rng.uniform(-c.sat, c.sat, (N, 1))
    sc = 1 + 0.1 * rng.standard_normal((B, 1))
    W, f = gc.weights_and_targets(rng, 4, B)
    w = rng.uniform(0.0, 2.0 / B, B) if weighted else None
    if what == "plant":
        op0 = (1 + 0.05 * rng.standard_normal((B, 1, 1))) * c.op0[None]

        def run(**kw):
            return m4q.plant_rollout_grad_batch(x0, u, op0, c.ops, c.dt, W, f, c.kind, u_scale=sc, figure=figure, **kw)
    else:
        models = gc.model_case(4, 1, 1, 1, 9701)[0][0][None] * (1 + 0.01 * rng.standard_normal((B, 1, 1)))

        def run(**kw):
            return m4q.model_rollout_grad_batch(x0, u, models, 1, W, f, u_scale=sc, figure=figure, **kw)
    full = run(scale_grad=True)
    red = run(reduce=True, weights=w, scale_grad=True)
    assert red["grad"].shape == (N, 1) and full["grad"].shape == (B, N, 1)
    assert np.array_equal(red["q"], full["q"]) and np.array_equal(red["grad_scale"], full["grad_scale"])
    assert np.array_equal(red["grad"], m4q.ordered_weighted_sum(full["grad"], w))
    assert red["q_mean"] == float(m4q.ordered_weighted_sum(_objectives(full["q"]), w))
    again = run(reduce=True, weights=w)
    assert np.array_equal(again["grad"], red["grad"]) and again["q_mean"] == red["q_mean"] and "grad_scale" not in again
    assert np.abs(red["grad"]).max() > 0


# ---------------------------------------------------------------- place and neighbours
PICK = (0, 1, 8191, 16384, 16388)


@pytest.mark.parametrize("what", ["plant", "model"])
def test_member_does_not_depend_on_its_place(what):
    B, N = 16389, 2                        # 4,098 quads - past the 4,096 workgroups the launch is capped at -, the last one ragged
    c = gc.plant_case("4-1")
    rng = np.random.default_rng(9800)
    x0 = np.ascontiguousarray(np.tile(c.states(rng, 64), (B // 64 + 1, 1))[:B] * (1 + 1e-3 * rng.standard_normal((B, 1))))
    u = rng.uniform(-c.sat, c.sat, (B, N, 1))
    sc = 1 + 0.1 * rng.standard_normal((B, 1))
    W, f = gc.weights_and_targets(rng, 4, B)
    pick = np.array(PICK)
    if what == "plant":
        op0 = (1 + 0.05 * rng.standard_normal((B, 1, 1))) * c.op0[None]
        ts = gc.grid(rng, N, c.dt)

        def run(idx):
            return m4q.plant_rollout_grad_batch(x0[idx], u[idx], op0[idx], c.ops, ts, W, f[idx], c.kind, u_scale=sc[idx], figure="sum",
                                                scale_grad=True)
    else:
        models = gc.model_case(4, 1, 1, 1, 9801)[0][0][None] * (1 + 0.01 * rng.standard_normal((B, 1, 1)))

        def run(idx):
            return m4q.model_rollout_grad_batch(x0[idx], u[idx], models[idx], 1, W, f[idx], u_scale=sc[idx], figure="sum", scale_grad=True)
    full = run(slice(None))
    five = run(pick)
    for key in ("q", "grad", "grad_scale"):
        assert np.isfinite(full[key]).all()
        assert np.array_equal(full[key][pick], five[key]), key
    assert len({full["grad"][b].tobytes() for b in PICK}) == len(PICK)                    # (the members do differ)


# ---------------------------------------------------------------- refusals
def test_generator_plant_is_refused():
    p = configs.build(3, batch=1)
    exp = m4q.QExperiment(p["plant_op0"][0], list(p["plant_ops"][0]))
    a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
    exp.set("c_ops", [0.2 * a])                                   # one collapse operator: operators() are Lindblad generators
    L0, Lk = exp.operators()
    assert exp.plant_kind == _lib.PLANT_GENERATOR and L0.shape == (9, 9)
    x0 = gc.plant_case("9-2").states(np.random.default_rng(9900), 2)
    with pytest.raises(_lib.M4qError) as err:
        m4q.plant_rollout_grad_batch(x0, np.zeros((3, 2)), L0, Lk, 0.25, np.eye(9), np.zeros(9), _lib.PLANT_GENERATOR)
    assert err.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.M4qError) as err:
        exp.gradient_batch(x0, np.arange(4) * 0.25, np.zeros((2, 4)), np.eye(9), np.zeros(9))
    assert err.value.code == _lib.E_UNSUPPORTED
    with pytest.raises(ValueError):
        m4q.LExperiment(L0, list(Lk)).gradient_batch(x0, np.arange(4) * 0.25, np.zeros((2, 4)), np.eye(9), np.zeros(9))


def test_experiment_wrappers_follow_the_module_functions():
    rng = np.random.default_rng(9901)
    ts = np.array([0.0, 0.2, 0.5, 0.55])
    for name in ("9-2", "16-1-process"):
        c = gc.plant_case(name)
        exp = (m4q.QSynthesis if c.kind == _lib.PLANT_PROCESS else m4q.QExperiment)(c.op0, list(c.ops))
        x0 = c.states(rng, 3)
        W, f = gc.weights_and_targets(rng, c.n, 3)
        us = rng.uniform(-c.sat, c.sat, (c.m, len(ts)))           # as simulate() takes them; the last column is unused
        sc = 1 + 0.1 * rng.standard_normal((3, c.m))
        got = exp.gradient_batch(x0, ts, us, W, f, u_scale=sc, figure="sum", scale_grad=True)
        want = m4q.plant_rollout_grad_batch(x0, us[:, :3].T, c.op0, c.ops, ts, W, f, c.kind, u_scale=sc, figure="sum", scale_grad=True)
        assert all(np.array_equal(got[k], want[k]) for k in ("q", "grad", "grad_scale"))
        sim = exp.simulate_batch(x0, ts, us, u_scale=sc, W=W, target=f, keep="none", figure="all")
        assert np.array_equal(got["q"], sim["q"])


# ---------------------------------------------------------------- descent
def test_projected_gradient_descent_lowers_the_ensemble_mean():
    """Config 1's plant, 64 detuned members, N = 20: five projected-gradient steps on |u| <= sat with backtracking on the reduced
    output.  Every accepted step lowers q_mean strictly."""
    p = configs.build(1)
    B, N = 64, 20
    rng = np.random.default_rng(9950)
    op0 = (1 + 0.2 * rng.standard_normal((B, 1, 1))) * p["plant_op0"][0][None]
    x0 = np.tile(p["x0"][:1], (B, 1))
    target = p["X_targ"][:, -1]
    W = p["Qf"].astype(complex)
    sat = p["sat"]

    def call(u):
        return m4q.plant_rollout_grad_batch(x0, u, op0, p["plant_ops"][0], p["dt"], W, target, reduce=True)
    u = np.full((N, 1), 0.1 * sat)
    cur = call(u)
    start = cur["q_mean"]
    step = 0.5 * sat / max(np.abs(cur["grad"]).max(), 1e-300)
    accepted = 0
    for _ in range(5):
        for _ in range(30):
            trial = np.clip(u - step * cur["grad"], -sat, sat)
            nxt = call(trial)
            if nxt["q_mean"] < cur["q_mean"]:
                break
            step *= 0.5
        else:
            raise AssertionError("no descent step found: the gradient is no descent direction")
        assert nxt["q_mean"] < cur["q_mean"]
        u, cur = trial, nxt
        accepted += 1
        print("step %d: q_mean = %.6f" % (accepted, cur["q_mean"]))
    assert accepted == 5 and cur["q_mean"] < start

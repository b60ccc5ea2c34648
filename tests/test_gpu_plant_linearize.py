"""The plant's own linearisation on the device (plant_linearize_kernel) against the NumPy / SciPy definition of
mpc4quantum_amd/plant_linearize.py, which tests/test_plant_linearize_host.py holds to the independent plant step and to central
differences; against the existing plant step and gradient kernels; and the feedback law built from it.  Tolerance of DESIGN
section 3: 1e-10 max(1, max|ref|).  Shapes are the smallest that can go wrong: B in {1, 5} (a ragged quad) and T in {1, 6}, so that
B T is neither a multiple of 4 nor aligned with members."""
import itertools

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd.vectorize import discretize_homogeneous, liouvillian
from tests import grad_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-10
U_TOL = 1e-10                                                       # the project's control tolerance
# what is shared by the ensemble and what is the member's own
#   shared  one operator set, one control sequence, u_scale, a non-uniform grid
#   per     per-member operators and control sequences, no u_scale, a scalar dt
RUNS = [("shared", 5, 6), ("per", 5, 6), ("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]
PLANTS = gc.PLANT_NAMES + ("16-2",)                                # the six cases and the plant-only shape
NAMES = ("A", "B", "Delta")


def _points(c, rng, B, T):
    """States that are not Hermitian and controls inside the bound."""
    X = c.states(rng, B * T).reshape(B, T, c.n)
    return X + 0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)), rng.uniform(-c.sat, c.sat, (B, T, c.m))


_FULL = {}


def _full(name):
    """Per-member everything at B = 5, T = 6 (u_scale, a non-uniform grid): the inputs and the device's answer, computed once."""
    if name not in _FULL:
        c = gc.plant_case(name)
        rng = np.random.default_rng(9800 + PLANTS.index(name))
        B, T = 5, 6
        X, U = _points(c, rng, B, T)
        op0, ops = c.member_ops(rng, B)
        sc = 1 + 0.1 * rng.standard_normal((B, c.m))
        ts = gc.grid(rng, T, c.dt)
        out = m4q.plant_linearize_batch(X, U, op0, ops, ts, c.kind, u_scale=sc)
        for a in (X, U, op0, ops, sc, ts) + out:
            a.setflags(write=False)
        _FULL[name] = (c, X, U, op0, ops, sc, ts, out)
    return _FULL[name]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.float64), b.view(np.float64))


@pytest.mark.parametrize("variant,B,T", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", PLANTS)
def test_against_the_definition(name, variant, B, T):
    c = gc.plant_case(name)
    rng = np.random.default_rng(9810 + 13 * PLANTS.index(name) + 101 * B + T)
    X, U = _points(c, rng, B, T)
    if variant == "per":
        op0, ops = c.member_ops(rng, B)
        ts, sc = c.dt, None
    else:
        op0, ops = c.op0, c.ops
        U, ts, sc = U[0], gc.grid(rng, T, c.dt), 1 + 0.1 * rng.standard_normal((B, c.m))
    ref = m4q.plant_linearize_reference(X, U, op0, ops, ts, c.kind, u_scale=sc)
    out = m4q.plant_linearize_batch(X, U, op0, ops, ts, c.kind, u_scale=sc)
    errs = []
    for what, got, want in zip(NAMES, out, ref):
        assert got.shape == want.shape and got.dtype == np.complex128 and np.isfinite(got).all()
        errs.append(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    print("%s %s B=%d T=%d: max|dA| %.2e, max|dB| %.2e (max|B_ref| = %.3e), max|dDelta| %.2e, each over max(1, max|ref|)"
          % (name, variant, B, T, errs[0], errs[1], np.abs(ref[1]).max(), errs[2]))
    assert max(errs) <= TOL
    assert np.abs(ref[1]).max() > 1e-3


@pytest.mark.parametrize("name", ["4-2", "9-2", "16-3", "16-1-process"])
def test_every_subset_of_the_outputs_gives_the_same_bits(name):
    c, X, U, op0, ops, sc, ts, full = _full(name)
    for r in (1, 2):
        for subset in itertools.combinations(NAMES, r):
            got = m4q.plant_linearize_batch(X, U, op0, ops, ts, c.kind, u_scale=sc, outputs=subset)
            for what, g, f in zip(NAMES, got, full):
                assert (g is None) if what not in subset else _bits(g, f)


@pytest.mark.parametrize("name", PLANTS)
def test_a_point_does_not_depend_on_its_place(name):
    """Member b alone gives the bits it gives inside B = 5; a point gives the same bits at t = 0 of a T = 1 call as at t = 3 of
    the T = 6 call with the same x, u and dt."""
    c, X, U, op0, ops, sc, ts, full = _full(name)
    for b in range(5):
        alone = m4q.plant_linearize_batch(X[b:b + 1], U[b:b + 1], op0[b], ops[b], ts, c.kind, u_scale=sc[b:b + 1])
        for g, f in zip(alone, full):
            assert _bits(g[0], f[b])
    one = m4q.plant_linearize_batch(X[:, 3:4], U[:, 3:4], op0, ops, ts[3:5], c.kind, u_scale=sc)
    for g, f in zip(one, full):
        assert _bits(g[:, 0], f[:, 3])


@pytest.mark.parametrize("name", PLANTS)
def test_against_the_plant_step_and_the_gradient_kernels(name):
    c, X, U, op0, ops, sc, ts, _ = _full(name)
    B, T, n = X.shape
    A, Bm, D = m4q.plant_linearize_batch(X, U, op0, ops, c.dt, c.kind, u_scale=sc)
    # A x + B u + Delta is the step of the existing plant kernel under the scaled controls
    rep = lambda a: np.repeat(a, T, axis=0)
    xn = m4q.plant_step_batch(X.reshape(B * T, n), (sc[:, None, :] * U).reshape(B * T, c.m), rep(op0), rep(ops), c.dt, c.kind).reshape(B, T, n)
    lin = np.einsum('btij,btj->bti', A, X) + np.einsum('btik,btk->bti', Bm, U) + D
    err = np.abs(lin - xn).max()
    print("%s: A x + B u + Delta against plant_step_batch %.2e (max|x| = %.3e)" % (name, err, np.abs(X).max()))
    assert err <= TOL * max(1.0, np.abs(X).max())
    # one step of the rollout gradient is the chain rule through B
    W, f = gc.weights_and_targets(np.random.default_rng(9850), n, B)
    g = m4q.plant_rollout_grad_batch(X[:, 0], U[:, :1], op0, ops, c.dt, W, f, c.kind, u_scale=sc)["grad"]
    lam = np.einsum('ij,bj->bi', W + W.conj().T, xn[:, 0] - f)
    chain = np.einsum('bi,bik->bk', lam.conj(), Bm[:, 0]).real
    err = np.abs(g[:, 0] - chain).max() / max(1.0, np.abs(g).max())
    print("%s: grad[b, 0, k] against Re(((W + W^H)(x_1 - f))^H B[:, k]) %.2e (max|g| = %.3e)" % (name, err, np.abs(g).max()))
    assert err <= TOL and np.abs(g).max() > 1e-3


@pytest.mark.parametrize("name", ["4-1", "9-2", "16-3"])
def test_the_law_of_the_plant_keeps_its_own_trajectory(name):
    """TVLQR around a plant trajectory with the trajectory itself as target: designed on the plant's Jacobians the law has no affine
    part and commands the nominal controls; designed on the order-1 model's it has (measured 0.11-0.57 on the device).  (The
    oracle's QP gives 2e-16 on the host for the former.)"""
    c = gc.plant_case(name)
    rng = np.random.default_rng(9860 + PLANTS.index(name))
    N, n, m = 8, c.n, c.m
    Q, R = np.identity(n), 0.1 * np.identity(m)
    x0 = c.states(rng, 1)
    U_nom = 0.5 * c.sat * rng.uniform(-1, 1, (N, m))
    X_nom = m4q.plant_rollout_batch(x0, U_nom, c.op0, c.ops, c.dt, c.kind)["xs"][0]
    law = m4q.FeedbackLaw.along_plant_trajectory(c.op0, c.ops, c.dt, X_nom, U_nom, X_nom, U_nom, Q, R, c.sat, kind=c.kind)
    assert law.gains.shape == (N, n + 1, m) and law.members is None
    affine = np.abs(law.gains[:, n, :]).max()
    run = m4q.plant_feedback_batch(x0, law, c.op0, c.ops, c.dt, c.kind)
    du = np.abs(run["us"][0] - U_nom).max()
    model = discretize_homogeneous([liouvillian(c.op0)] + [liouvillian(h) for h in c.ops], c.dt, 1)
    model_law = m4q.FeedbackLaw.along_trajectory(model, 1, X_nom, U_nom, X_nom, U_nom, Q, R, c.sat)
    model_affine = np.abs(model_law.gains[:, n, :]).max()
    print("%s: affine column %.2e (max|K| = %.3e), max|us - U_nom| %.2e; order-1 model's affine column %.2e"
          % (name, affine, np.abs(law.gains[:, :n]).max(), du, model_affine))
    assert affine <= U_TOL
    assert du <= U_TOL and np.array_equal(run["clipped"], [0]) and np.array_equal(run["status"], [0])
    assert model_affine > 1e-2
    assert np.abs(law.gains[:, :n]).max() > 1e-2              # (a law that reacts: not the zero gains of a flat problem)


@pytest.mark.parametrize("name", ["4-1", "9-2", "16-3"])
def test_a_per_member_law_is_each_member_s_own(name):
    c = gc.plant_case(name)
    rng = np.random.default_rng(9870 + PLANTS.index(name))
    B, N, n, m = 5, 8, c.n, c.m
    Q, R = np.identity(n), 0.1 * np.identity(m)
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    ts = gc.grid(rng, N, c.dt)
    U_nom = 0.5 * c.sat * rng.uniform(-1, 1, (B, N, m))
    u_prev = 0.5 * c.sat * rng.uniform(-1, 1, (B, m))
    X_nom = m4q.plant_rollout_batch(x0, U_nom, op0, ops, ts, c.kind, u_scale=sc)["xs"]
    X_targ = X_nom[0] + 0.02                                   # one shared target off every nominal: the affine column works
    args = (Q, R, c.sat, 0.8 * c.sat)
    law = m4q.FeedbackLaw.along_plant_trajectory(op0, ops, ts, X_nom, U_nom, X_targ, U_nom, *args, u_prev=u_prev, kind=c.kind, u_scale=sc)
    assert law.gains.shape == (B, N, n + 1, m) and law.members == B and law.prev_members == B
    assert _bits(law.x_ref, np.broadcast_to(X_targ[:N], (B, N, n)).copy()) and _bits(law.u_ref, U_nom)
    worst = 0.0
    for b in range(B):
        own = m4q.FeedbackLaw.along_plant_trajectory(op0[b], ops[b], ts, X_nom[b], U_nom[b], X_targ, U_nom[b], *args, u_prev=u_prev[b],
                                                     kind=c.kind, u_scale=sc[b:b + 1])
        assert own.members is None
        worst = max(worst, np.abs(own.gains - law.gains[b]).max() / max(1.0, np.abs(own.gains).max()))
    print("%s: per-member law against each member's own %.2e (max|gains| = %.3e)" % (name, worst, np.abs(law.gains).max()))
    assert worst <= TOL and np.abs(law.gains[:, :, n]).max() > 1e-3
    # and it runs: the members' plants under their own laws, in one launch
    run = m4q.plant_feedback_batch(x0, law, op0, ops, ts, c.kind, u_scale=sc)
    assert np.array_equal(run["status"], np.zeros(B, np.int32)) and np.isfinite(run["xs"]).all()


def test_the_experiment_wrappers_return_the_module_function_s_arrays():
    c, X, U, op0, ops, sc, ts, _ = _full("9-2")
    want = m4q.plant_linearize_batch(X, U, c.op0, c.ops, ts, c.kind, u_scale=sc)
    got = m4q.QExperiment(c.op0, list(c.ops)).linearize_batch(X, U, ts, u_scale=sc)
    assert all(_bits(g, w) for g, w in zip(got, want))
    want = m4q.plant_linearize_batch(X, U, op0, c.ops, ts, c.kind, outputs=("B", "Delta"))
    got = m4q.QExperiment(c.op0, list(c.ops)).linearize_batch(X, U, ts, outputs=("B", "Delta"), op0=op0)
    assert got[0] is None and _bits(got[1], want[1]) and _bits(got[2], want[2])
    c, X, U, op0, ops, sc, ts, _ = _full("16-1-process")
    want = m4q.plant_linearize_batch(X, U, c.op0, c.ops, ts, c.kind, u_scale=sc)
    got = m4q.QSynthesis(c.op0, list(c.ops)).linearize_batch(X, U, ts, u_scale=sc)
    assert all(_bits(g, w) for g, w in zip(got, want))

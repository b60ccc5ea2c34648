"""What the tests of the robust optimiser share (tests/test_plant_robust_host.py, tests/test_gpu_plant_robust.py): seeded ensembles on
tests/grad_cases.py's PlantCase - per-member operators, u_scale and targets, a non-Hermitian W, a non-uniform grid, unequal weights -
and the pair of callables that drives plant_robust_reference from the package's existing device entry points."""
import numpy as np

import mpc4quantum_amd as m4q
from tests import grad_cases as gc

NAMES = ("4-1", "9-2", "16-3", "16-1-process")
STEP0 = 0.05


def case(name, B, N, seed):
    """One seeded ensemble: the positional arguments of plant_robust_batch / plant_robust_reference up to sat, and the keywords."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(seed)
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    W, f = gc.weights_and_targets(rng, c.n, B)
    ts = gc.grid(rng, N, c.dt)
    w = rng.uniform(0.5, 1.5, B)
    U0 = rng.uniform(-0.5 * c.sat, 0.5 * c.sat, (N, c.m))
    return dict(c=c, args=(x0, U0, op0, ops, ts, W, f, c.sat), kw=dict(kind=c.kind, u_scale=sc, weights=w / w.sum()))


def own_trajectory_case(name="4-1", N=5, seed=4500):
    """Status 2: one member, W = 1, target = its own final state under U0 (by the independent chain: equal to rounding), so that F
    is a sum of squared rounding errors and every trial step of length step0 raises it."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(seed)
    x0 = c.states(rng, 1)
    U0 = rng.uniform(-0.5 * c.sat, 0.5 * c.sat, (N, c.m))
    ts = gc.grid(rng, N, c.dt)
    f = gc.plant_chain(c, x0[0], U0, c.op0, c.ops, np.diff(ts))[-1]
    f = f * (1 + 1e-9)                                              # (never exactly the definition's own x_N: a zero gradient is status 1)
    return (x0, U0, c.op0, c.ops, ts, np.eye(c.n), f, c.sat), dict(kind=c.kind, iters=4, steps=2, mem=3, step0=0.1, tol=0.0, gtol=0.0)


def reference_evaluate(k, figure):
    """(grad_fn, roll_fn) on the NumPy definitions - what plant_robust_reference builds for itself when evaluate is None."""
    x0, _, op0, ops, ts, W, f, _ = k["args"]
    kw = dict(k["kw"], figure=figure)

    def grad_fn(U):
        out = m4q.plant_rollout_grad_reference(x0, U, op0, ops, ts, W, f, reduce=True, **kw)
        return out["q_mean"], out["grad"]

    def roll_fn(us, members=False):
        out = m4q.plant_rollout_multi_reference(x0, us, op0, ops, ts, W, f, **kw)
        return (out["F"], out["J"]) if members else out["F"]
    return grad_fn, roll_fn


# The device's gradient may differ from the definition's by the project's gradient bound, 1e-10 max(1, max|g|).
# How far that can move the optimiser is measured on the definition itself: the same run with every entry of every gradient pushed
# by that bound, signs seeded.
GRAD_BOUND = 1e-10
PARITY = dict(B=11, N=6, iters=3, steps=4)
_RUNS = {}


def perturbed(grad_fn, seed):
    rng = np.random.default_rng(seed)

    def fn(U):
        F, g = grad_fn(U)
        g = np.asarray(g)
        return F, g + GRAD_BOUND * max(1.0, np.abs(g).max()) * rng.choice([-1.0, 1.0], g.shape)
    return fn


def parity_case(name):
    return case(name, PARITY["B"], PARITY["N"], 9300 + 11 * NAMES.index(name))


def definition_runs(name, figure, mem):
    """(plain, pushed): plant_robust_reference on the parity case, and the same with its gradients pushed by GRAD_BOUND.
    Computed once per (name, figure, mem)."""
    key = (name, figure, mem)
    if key not in _RUNS:
        k = parity_case(name)
        kw = dict(iters=PARITY["iters"], steps=PARITY["steps"], mem=mem, step0=STEP0, tol=0.0)
        grad_fn, roll_fn = reference_evaluate(k, figure)
        plain = m4q.plant_robust_reference(*k["args"], figure=figure, **k["kw"], **kw)
        pushed = m4q.plant_robust_reference(*k["args"], figure=figure, **k["kw"], **kw,
                                            evaluate=(perturbed(grad_fn, 77 + NAMES.index(name)), roll_fn))
        _RUNS[key] = (plain, pushed)
    return _RUNS[key]


def movement(plain, pushed):
    """max |U - U'| and max |cost_hist - cost_hist'| between two runs."""
    return float(np.abs(plain["U"] - pushed["U"]).max()), float(np.abs(plain["cost_hist"] - pushed["cost_hist"]).max())


def device_evaluate(k, figure):
    """(grad_fn, roll_fn) of plant_robust_reference(evaluate=...) on plant_rollout_grad_batch(reduce=True) and plant_rollout_batch:
    the loop composed from the entry points the package had before the one call."""
    x0, _, op0, ops, ts, W, f, _ = k["args"]
    kind, sc, w = k["kw"]["kind"], k["kw"]["u_scale"], k["kw"]["weights"]

    def grad_fn(U):
        out = m4q.plant_rollout_grad_batch(x0, U, op0, ops, ts, W, f, kind, u_scale=sc, figure=figure, weights=w, reduce=True)
        return out["q_mean"], out["grad"]

    def roll_fn(us, members=False):
        J = np.stack([member_objectives(k, u, figure) for u in us], axis=1)
        F = m4q.ordered_weighted_sum(J, w)
        return (F, J) if members else F
    return grad_fn, roll_fn


def member_objectives(k, u, figure):
    """J [B] under the shared sequence u [N, m] from plant_rollout_batch's figure: q_N, or its columns added with t ascending."""
    x0, _, op0, ops, ts, W, f, _ = k["args"]
    q = m4q.plant_rollout_batch(x0, u, op0, ops, ts, k["kw"]["kind"], u_scale=k["kw"]["u_scale"], W=W, target=f, keep="none",
                                figure="all" if figure == "sum" else "last")["q"]
    if figure == "last":
        return q
    J = np.zeros(q.shape[0])
    for t in range(q.shape[1]):
        J = J + q[:, t]
    return J

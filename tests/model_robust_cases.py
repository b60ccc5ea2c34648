"""What the tests of the robust optimiser on models share (tests/test_model_robust_host.py, tests/test_gpu_model_robust.py): seeded
ensembles on tests/grad_cases.py's model_case - per-member models, u_scale and targets, a non-Hermitian W, unequal weights - the
pairs of callables that drive the loop from the NumPy definitions and from the package's earlier device entry points, and the
dissipative qubit both files optimise a pulse for."""
import numpy as np

import mpc4quantum_amd as m4q
from mpc4quantum_amd.configs import SX, SZ
from tests import grad_cases as gc
from tests import plant_robust_cases as rc

SHAPES = gc.MODEL_SHAPES
PARITY = rc.PARITY                                   # B = 11, N = 6, 3 iterations, 4 candidates
MEMS, FIGURES = (0, 3), ("last", "sum")
# The seed of a cell is 9400 + 11 i.  One cell - (16, 1, 4), "sum", mem 3 - ends with every entry of U on the box under that seed:
# the pushed gradient then moves U by exactly 0, which says nothing about how far a gradient error may move the optimiser.  Its seed
# was chosen on the definition: the first of 9400 + 11 i + 1000 j, j = 1, 2, ..., with identical decisions and a non-zero movement
# (j = 1, 2 move U by 0 as well).  The run under the original seed - a status 1 - stays in the host test, for its decisions.
RESEEDED = {((16, 1, 4), "sum", 3): 12444}
_RUNS = {}


def seed_of(shape, figure, mem):
    return RESEEDED.get((tuple(shape), figure, mem), 9400 + 11 * SHAPES.index(tuple(shape)))


def case(shape, B, N, seed):
    """One seeded ensemble: the positional arguments of model_robust_batch / model_robust_reference up to sat, and the keywords."""
    n, m, order = shape
    models, x0, sat, rng = gc.model_case(n, m, order, B, seed)
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    W, f = gc.weights_and_targets(rng, n, B)
    w = rng.uniform(0.5, 1.5, B)
    U0 = rng.uniform(-0.5 * sat, 0.5 * sat, (N, m))
    return dict(shape=tuple(shape), args=(x0, U0, models, order, W, f, sat), kw=dict(u_scale=sc, weights=w / w.sum()))


def parity_case(shape, figure, mem, seed=None):
    return case(shape, PARITY["B"], PARITY["N"], seed_of(shape, figure, mem) if seed is None else seed)


def reference_evaluate(k, figure):
    """(grad_fn, roll_fn) on the NumPy definitions - what model_robust_reference builds for itself when evaluate is None."""
    x0, _, models, order, W, f, _ = k["args"]
    kw = dict(k["kw"], figure=figure)

    def grad_fn(U):
        out = m4q.model_rollout_grad_reference(x0, U, models, order, W, f, reduce=True, **kw)
        return out["q_mean"], out["grad"]

    def roll_fn(us, members=False):
        out = m4q.model_rollout_multi_reference(x0, us, models, order, W, f, **kw)
        return (out["F"], out["J"]) if members else out["F"]
    return grad_fn, roll_fn


def definition_runs(shape, figure, mem, seed=None):
    """(plain, pushed): model_robust_reference on the parity case, and the same with every gradient pushed by the project's
    gradient bound (plant_robust_cases.perturbed).  Computed once per cell (and seed, where one is given in place of the cell's)."""
    key = (tuple(shape), figure, mem, seed)
    if key not in _RUNS:
        k = parity_case(shape, figure, mem, seed)
        kw = dict(iters=PARITY["iters"], steps=PARITY["steps"], mem=mem, step0=rc.STEP0, tol=0.0)
        grad_fn, roll_fn = reference_evaluate(k, figure)
        plain = m4q.model_robust_reference(*k["args"], figure=figure, **k["kw"], **kw)
        pushed = m4q.model_robust_reference(*k["args"], figure=figure, **k["kw"], **kw,
                                            evaluate=(rc.perturbed(grad_fn, 77 + SHAPES.index(tuple(shape))), roll_fn))
        _RUNS[key] = (plain, pushed)
    return _RUNS[key]


def member_objectives(k, u, figure):
    """J [B] under the shared sequence u [N, m] from model_rollout_batch's figure: q_N, or its columns added with t ascending."""
    x0, _, models, order, W, f, _ = k["args"]
    q = m4q.model_rollout_batch(x0, u, models, order, u_scale=k["kw"]["u_scale"], W=W, target=f, keep="none",
                                figure="all" if figure == "sum" else "last")["q"]
    if figure == "last":
        return q
    J = np.zeros(q.shape[0])
    for t in range(q.shape[1]):
        J = J + q[:, t]
    return J


def device_evaluate(k, figure):
    """(grad_fn, roll_fn) on model_rollout_grad_batch(reduce=True) and model_rollout_batch per candidate: the loop composed from
    the entry points the package had before the one call."""
    x0, _, models, order, W, f, _ = k["args"]
    sc, w = k["kw"]["u_scale"], k["kw"]["weights"]

    def grad_fn(U):
        out = m4q.model_rollout_grad_batch(x0, U, models, order, W, f, u_scale=sc, figure=figure, weights=w, reduce=True)
        return out["q_mean"], out["grad"]

    def roll_fn(us, members=False):
        J = np.stack([member_objectives(k, u, figure) for u in us], axis=1)
        F = m4q.ordered_weighted_sum(J, w)
        return (F, J) if members else F
    return grad_fn, roll_fn


def own_trajectory_case(shape=(4, 1, 1), N=5, seed=4500):
    """Status 2 (plant_robust_cases.own_trajectory_case on a model): one member, W = 1, target = its own final state under U0 by
    the independent chain, a hair off: F is a sum of squared rounding errors and every trial step of length step0 raises it."""
    n, m, order = shape
    models, x0, sat, rng = gc.model_case(n, m, order, 1, seed)
    U0 = rng.uniform(-0.5 * sat, 0.5 * sat, (N, m))
    f = gc.model_chain(models[0], m, order, x0[0], U0)[-1] * (1 + 1e-9)
    return (x0, U0, models, order, np.eye(n), f, sat), dict(iters=4, steps=2, mem=3, step0=0.1, tol=0.0, gtol=0.0)


# ---------------------------------------------------------------- the dissipative qubit
DISSIPATIVE = dict(B=8, N=12, dt=0.5, sat=2 * np.pi * 0.1, iters=8, steps=6, mem=5, step0=0.1, tol=0.0)


def dissipative_case():
    """A qubit with dephasing, an ensemble of 8 detuned members: the experiment, x0 [B, 4], U0 [N, 1], the members' generators
    L0 [B, 4, 4] - the drift of the Hamiltonian part scaled member by member, the dissipator shared; what a QExperiment with
    collapse operators takes as op0 -, the control generator, u_scale, W and the target."""
    d = DISSIPATIVE
    H0, H1, c = 0.15 * SZ, 0.5 * SX, np.sqrt(0.02) * SZ
    rng = np.random.default_rng(4600)
    xi, zeta = rng.standard_normal(d["B"]), rng.standard_normal((d["B"], 1))
    exp = m4q.QExperiment(H0, [H1])
    exp.set("c_ops", [c])
    L0_own, Lk = exp.operators()
    diss = L0_own - m4q.liouvillian(H0)                            # the dissipator: the same for every member
    L0 = np.stack([(1 + 0.05 * s) * m4q.liouvillian(H0) + diss for s in xi])
    x0 = np.tile(np.array([1, 0, 0, 0], dtype=complex), (d["B"], 1))
    target = np.array([0, 0, 0, 1], dtype=complex)
    U0 = np.full((d["N"], 1), 0.3 * d["sat"])
    return dict(exp=exp, x0=x0, U0=U0, L0=L0, L1=Lk[0], u_scale=1 + 0.02 * zeta, W=np.eye(4, dtype=complex), target=target)


def generator_plant_mean(c, U):
    """The generator plant's own ensemble mean of q_N under U [N, 1]: SciPy's expm of dt (L0_b + s_b u L_1), member by member."""
    from scipy.linalg import expm
    d = DISSIPATIVE
    q = np.empty(d["B"])
    for b in range(d["B"]):
        x = c["x0"][b]
        for t in range(d["N"]):
            x = expm(d["dt"] * (c["L0"][b] + c["u_scale"][b, 0] * U[t, 0] * c["L1"])) @ x
        e = x - c["target"]
        q[b] = np.real(e.conj() @ (c["W"] @ e))
    return float(m4q.ordered_weighted_sum(q))

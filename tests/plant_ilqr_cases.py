"""What the tests of the iLQR on the plant itself share (tests/test_plant_ilqr_host.py, tests/test_gpu_plant_ilqr.py): the cells, runs
and seeded inputs of tests/plant_sqp_cases.py - the two methods are run on the same problems - with this file's own seed shifts, the
definition's answers (computed once, left unchanged) and the recorded amplification of every case."""
import numpy as np

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd.feedback import _plant_step
from tests import grad_cases as gc
from tests import plant_sqp_cases as _sqp
from tests.plant_sqp_cases import CELLS, MARGIN, RUNS, STEPS, TOL_SQP, bounds, margins  # noqa: F401
from tests.plant_sqp_cases import problem as _sqp_problem

EPS = _sqp.EPS
case_id, all_cases = _sqp.case_id, _sqp.all_cases

# At three iterations the clipped case of this run has two candidates 1.1e-7 of J apart on the SQP's seed: the run takes the first
# seed whose decisions all pass MARGIN (tests/test_plant_ilqr_host.py::test_decision_margins_of_the_gpu_cases), as
# plant_sqp_cases.SEED_SHIFT does for its own.
SEED_SHIFT = {("4-2", "shared", 5, 1): 1}
_PROBLEMS = {}


def draw(name, variant, B, T, shift):
    """plant_sqp_cases.problem's draw (see there for what a run is) with the seed shift an argument: that builder reads its own
    module's table, which this file leaves alone.  tests/test_plant_ilqr_host.py holds the two draws together at the SQP's shifts."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(7300 + 13 * CELLS.index(name) + 101 * B + T + (50 if variant == "per" else 0) + 1000 * shift)
    x0 = c.states(rng, B)
    dt = _sqp.ANGLE / (c.sat * np.linalg.norm(c.ops[0], 2))
    U0 = 0.5 * c.sat * rng.uniform(-1, 1, (B, T, c.m))
    U_to = 0.9 * c.sat * rng.uniform(-1, 1, (B, T, c.m))
    if variant == "per":
        op0, ops = c.member_ops(rng, B)
        ts, sc = dt, None
    else:
        op0, ops = c.op0, c.ops
        U0, ts, sc = U0[0], gc.grid(rng, T, dt), 1 + 0.1 * rng.standard_normal((B, c.m))
    dts = np.full(T, ts) if np.ndim(ts) == 0 else np.diff(ts)
    xs = np.empty((B, T + 1, c.n), dtype=complex)
    far = c.states(rng, B)
    for b in range(B if variant == "per" else 1):
        xs[b, 0] = far[b]
        for t in range(T):
            xs[b, t + 1] = _plant_step(c.kind, xs[b, t], U_to[b, t], op0[b] if variant == "per" else op0,
                                       ops[b] if variant == "per" else ops, dts[t])
    shift_x = 0.03 * rng.uniform(0.5, 1.5, (T + 1, 1))
    X_bm = xs + shift_x if variant == "per" else xs[0] + shift_x
    U_bm = np.zeros((B, T, c.m)) if variant == "per" else np.zeros((T, c.m))
    kw = dict(kind=c.kind, u_scale=sc, steps=STEPS, tol=TOL_SQP)
    if variant == "per":
        kw.update(du=0.5 * c.sat, u_prev=0.3 * c.sat * rng.uniform(-1, 1, (B, c.m)))
    args = (x0, U0, op0, ops, ts, X_bm, U_bm, np.identity(c.n), 0.1 * np.identity(c.m), c.sat)
    for a in args[:-1]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, args, kw


def problem(name, variant, B, T):
    """plant_sqp_cases.problem(...) - the SQP's own object - but for the runs SEED_SHIFT names, which are drawn here."""
    key = (name, variant, B, T)
    if key not in SEED_SHIFT:
        return _sqp_problem(*key)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = draw(*key, SEED_SHIFT[key])
    return _PROBLEMS[key]


_REFS = {}


def reference(name, variant, B, T, exact, iters):
    """The definition's answer (with gains) and its trace, computed once."""
    key = (name, variant, B, T, exact, iters)
    if key not in _REFS:
        c, args, kw = problem(name, variant, B, T)
        trace = []
        ref = m4q.plant_ilqr_reference(*args, iters=iters, exact=exact, gains=True, trace=trace, **kw)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = (ref, trace)
    return _REFS[key]


_CONVERGED = {}


NARROW = 0.05                                                      # the narrow box of converged_start, as a part of the run's


def converged_start(name="4-2", B=3, T=6, exact=True, box=1.0):
    """A start from the definition's own converged point: run with tol = 0 (so that only 'no candidate lowers the cost' stops a
    member) until every member has stopped that way.  box scales the run's bound on the controls: in a box of NARROW the
    minimiser has nearly every control on a bound, and a member all of whose controls the exact QP pins has the iterate itself
    for every candidate.  Returns (c, args with U0 replaced, kw, exact)."""
    key = (name, B, T, exact, box)
    if key not in _CONVERGED:
        c, args, kw = problem(name, "per", 5, T)                   # (its first B members)
        args = tuple(a[:B] if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a for a in args[:9]) + (box * args[9],)
        kw = dict(kw, u_prev=kw["u_prev"][:B])
        U = args[1]
        for _ in range(12):
            out = m4q.plant_ilqr_reference(args[0], U, *args[2:], iters=64, exact=exact, **dict(kw, tol=0.0))
            U = out["U"]
            if np.all(out["status"] == 2):
                break
        assert np.all(out["status"] == 2), out["status"]
        U = np.ascontiguousarray(U)
        U.setflags(write=False)
        _CONVERGED[key] = (c, (args[0], U) + args[2:], kw, exact)
    return _CONVERGED[key]


def held_members(args, kw, exact):
    """The members of a start every candidate of whose first iteration is the iterate bit for bit in the definition (every
    control pinned: ff = U_qp - U = 0, no feedback): their candidates have the iterate's cost bit for bit on the device as in the
    definition - one arithmetic on one input - so status 2 is no rounding decision for them (plant_sqp_cases.margins)."""
    trace = []
    m4q.plant_ilqr_reference(*args, iters=1, exact=exact, trace=trace, **kw)
    held = np.zeros(args[0].shape[0], dtype=bool)
    for rec in trace:
        held[rec["b"]] = all(np.array_equal(u, rec["U"]) for u in rec["Us"])
    return held


def move_bounds(args, kw, J):
    """How far a step accepted from a converged start of the definition can move a member's controls and states, [B] each.
    The definition found no lower cost at any step length down to a = 2^-(steps-1).  Along the QP's step d the model falls by
    a (1 - a/2) h, h = d'Hd >= lambda_min(R) |d|^2 (Gauss-Newton: H = R + what the states add, on the free controls; a pinned one
    does not move), so h <= 2^steps e J, e the relative rounding of a cost - a sum of T (n + m) squares, each a rounded sum of its
    own: 2 T (n + m) epsilon.  A candidate moves the controls by a d + O(|d|^2) (on a linear plant the law reproduces the line),
    and the device's d is the definition's to ~1e-12; a factor 2 covers both:  |U - U0| <= 2 sqrt(2^steps e J / lambda_min(R)).
    A Hamiltonian step is unitary, and a change du of its controls moves its state by at most dt sum_k |du_k| |H_k| |x|, so over
    T steps |X - X(U0)| <= T dt sum_k |H_k| |x0| max|U - U0|.  (The "per" runs: a scalar dt, no u_scale.)"""
    x0, U0, op0, ops, dt, R = args[0], args[1], args[2], args[3], args[4], args[8]
    assert kw["kind"] == _lib.PLANT_HAMILTONIAN and kw["u_scale"] is None and np.ndim(dt) == 0 and ops.ndim == 4
    (B, n), (T, m) = x0.shape, U0.shape[-2:]
    e = 2 * T * (n + m) * np.finfo(float).eps
    dU = 2 * np.sqrt(2.0 ** kw["steps"] * e * J / np.linalg.eigvalsh(R).min())
    dX = np.array([T * dt * sum(np.linalg.norm(H, 2) for H in ops[b]) * np.linalg.norm(x0[b]) for b in range(B)]) * dU
    return dU, dX


# The definition's amplification, case by case, as (at iters = 1, at iters = 3): the largest relative change of any output (over
# max(1, max|output|)) under random relative perturbations of 1e-12 of x0, U0 and the operators, over 1e-12.  Recorded by
# tests/test_plant_ilqr_host.py::test_amplification_of_the_gpu_cases, which prints the table; the GPU file's bound at either
# iteration count is TOL max(1, 10 s).
AMPLIFICATION = {
    "4-1/shared-5-6/clipped": (2.6, 3.6), "4-1/shared-5-6/exact": (3.5, 8.2), "4-1/per-5-6/clipped": (30.9, 30.3),
    "4-1/per-5-6/exact": (8.5, 21.3), "4-1/shared-5-1/clipped": (3.9, 2.5), "4-1/shared-5-1/exact": (1.6, 1.6),
    "4-1/per-1-1/clipped": (0.9, 0.9), "4-1/per-1-1/exact": (1.0, 1.0), "4-1/shared-1-6/clipped": (1.7, 1.5),
    "4-1/shared-1-6/exact": (1.1, 1.7), "4-2/shared-5-6/clipped": (291.0, 4206.9), "4-2/shared-5-6/exact": (57.6, 369.1),
    "4-2/per-5-6/clipped": (52.0, 2576.3), "4-2/per-5-6/exact": (10.9, 29.6), "4-2/shared-5-1/clipped": (14.4, 16.6),
    "4-2/shared-5-1/exact": (31.8, 16.7), "4-2/per-1-1/clipped": (0.3, 0.7), "4-2/per-1-1/exact": (2.4, 3.3),
    "4-2/shared-1-6/clipped": (35.1, 83.4), "4-2/shared-1-6/exact": (6.8, 30.9), "9-2/shared-5-6/clipped": (2.5, 3.6),
    "9-2/shared-5-6/exact": (3.5, 3.6), "9-2/per-5-6/clipped": (9.1, 12.3), "9-2/per-5-6/exact": (6.2, 7.6),
    "9-2/shared-5-1/clipped": (2.0, 2.1), "9-2/shared-5-1/exact": (1.7, 1.7), "9-2/per-1-1/clipped": (1.2, 1.2),
    "9-2/per-1-1/exact": (0.9, 0.9), "9-2/shared-1-6/clipped": (2.6, 2.2), "9-2/shared-1-6/exact": (4.9, 8.3),
    "16-1/shared-5-6/clipped": (18.3, 75.2), "16-1/shared-5-6/exact": (31.1, 33.2), "16-1/per-5-6/clipped": (22.9, 69.4),
    "16-1/per-5-6/exact": (12.0, 14.6), "16-1/shared-5-1/clipped": (1.1, 0.7), "16-1/shared-5-1/exact": (1.0, 1.6),
    "16-1/per-1-1/clipped": (1.4, 1.0), "16-1/per-1-1/exact": (0.9, 0.8), "16-1/shared-1-6/clipped": (29.9, 18.7),
    "16-1/shared-1-6/exact": (30.2, 29.1), "16-1-process/shared-5-6/clipped": (1.4, 1.7),
    "16-1-process/shared-5-6/exact": (1.2, 1.7), "16-1-process/per-5-6/clipped": (1.3, 2.8),
    "16-1-process/per-5-6/exact": (1.9, 2.0), "16-1-process/shared-5-1/clipped": (0.9, 0.9),
    "16-1-process/shared-5-1/exact": (1.0, 1.1), "16-1-process/per-1-1/clipped": (0.6, 0.6),
    "16-1-process/per-1-1/exact": (0.7, 0.7), "16-1-process/shared-1-6/clipped": (1.4, 0.9),
    "16-1-process/shared-1-6/exact": (1.8, 1.5), "16-3/shared-5-6/clipped": (37.4, 72.7), "16-3/shared-5-6/exact": (141.9, 447.6),
    "16-3/per-5-6/clipped": (43.6, 41.2), "16-3/per-5-6/exact": (22.3, 37.6), "16-3/shared-5-1/clipped": (4.5, 2.9),
    "16-3/shared-5-1/exact": (3.1, 5.7), "16-3/per-1-1/clipped": (1.9, 13.1), "16-3/per-1-1/exact": (2.9, 11.9),
    "16-3/shared-1-6/clipped": (59.1, 29.5), "16-3/shared-1-6/exact": (28.1, 18.8), "16-3-process/shared-5-6/clipped": (2.1, 7.8),
    "16-3-process/shared-5-6/exact": (2.0, 7.0), "16-3-process/per-5-6/clipped": (3.8, 13.3),
    "16-3-process/per-5-6/exact": (2.5, 5.2), "16-3-process/shared-5-1/clipped": (1.1, 2.9),
    "16-3-process/shared-5-1/exact": (1.6, 5.9), "16-3-process/per-1-1/clipped": (1.6, 1.2),
    "16-3-process/per-1-1/exact": (1.4, 1.0), "16-3-process/shared-1-6/clipped": (1.6, 1.7),
    "16-3-process/shared-1-6/exact": (7.1, 1.4),
}

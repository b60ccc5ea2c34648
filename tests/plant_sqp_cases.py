"""What the tests of the SQP on the plant itself share (tests/test_plant_sqp_host.py, tests/test_gpu_plant_sqp.py): the cells, the
runs, seeded inputs built on the host alone, the definition's answers (computed once, left unchanged), the decision margins of
those answers and the recorded amplification of every case."""
import numpy as np

import mpc4quantum_amd as m4q
from mpc4quantum_amd.feedback import _plant_step
from tests import grad_cases as gc

# every (shape, plant) launch_plant_qp is built for: tests/test_gpu_plant_qp.py: _cells() (the GPU file asserts the two agree)
CELLS = ["4-1", "4-2", "9-2", "16-1", "16-1-process", "16-3", "16-3-process"]
RUNS = [("shared", 5, 6), ("per", 5, 6), ("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]
STEPS = 4
TOL_SQP = 1e-9                                                     # the loop's own tol in every GPU case
MARGIN = 1e-6
EPS = 1e-12                                                        # the relative perturbation of the amplification record
ANGLE = 1.2                                                        # radians a control at its bound turns the plant by in one step


def case_id(name, variant, B, T, exact):
    return "%s/%s-%d-%d/%s" % (name, variant, B, T, "exact" if exact else "clipped")


def all_cases():
    return [(name, variant, B, T, exact) for name in CELLS for variant, B, T in RUNS for exact in (False, True)]


_PROBLEMS = {}
# One control over one step is a problem in one unknown, on which Gauss-Newton is within 1e-6 of its limit by the third iteration
# for most draws: these runs take the first seed whose three iterations all decide by more than MARGIN (test_decision_margins...).
SEED_SHIFT = {("4-1", "shared", 5, 1): 3, ("4-1", "per", 1, 1): 1, ("16-1", "shared", 5, 1): 12}


def problem(name, variant, B, T):
    """One run's inputs: (c, args, kw) with plant_sqp_batch(*args, **kw).
      shared  one operator set, one first guess, u_scale, a non-uniform grid, one target
      per     per-member operators, first guesses and targets, a scalar dt, the du band around per-member u_prev
    The step length makes a control at its bound turn the plant by ANGLE per step, and the targets are the plant's trajectories
    from OTHER states under other random controls, shifted: nonlinear problems with a large residual, on which three Gauss-Newton
    iterations are still far from their limit and every decision has a margin.  Q = I, R = 0.1 I; first guesses at half the bound."""
    key = (name, variant, B, T)
    if key not in _PROBLEMS:
        c = gc.plant_case(name)
        rng = np.random.default_rng(7300 + 13 * CELLS.index(name) + 101 * B + T + (50 if variant == "per" else 0)
                                    + 1000 * SEED_SHIFT.get(key, 0))
        x0 = c.states(rng, B)
        dt = ANGLE / (c.sat * np.linalg.norm(c.ops[0], 2))
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
        shift = 0.03 * rng.uniform(0.5, 1.5, (T + 1, 1))
        X_bm = xs + shift if variant == "per" else xs[0] + shift
        U_bm = np.zeros((B, T, c.m)) if variant == "per" else np.zeros((T, c.m))
        Q, R = np.identity(c.n), 0.1 * np.identity(c.m)
        kw = dict(kind=c.kind, u_scale=sc, steps=STEPS, tol=TOL_SQP)
        if variant == "per":
            kw.update(du=0.5 * c.sat, u_prev=0.3 * c.sat * rng.uniform(-1, 1, (B, c.m)))
        args = (x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, c.sat)
        for a in args[:-1]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _PROBLEMS[key] = (c, args, kw)
    return _PROBLEMS[key]


def bounds(args, kw):
    """lo, hi [B, T, m] of a problem."""
    x0, U0 = args[0], args[1]
    B, (T, m), sat = x0.shape[0], U0.shape[-2:], args[9]
    lo, hi = np.full((B, T, m), -sat), np.full((B, T, m), sat)
    if kw.get("du") is not None:
        lo[:, 0], hi[:, 0] = np.maximum(lo[:, 0], kw["u_prev"] - kw["du"]), np.minimum(hi[:, 0], kw["u_prev"] + kw["du"])
    return lo, hi


_REFS = {}


def reference(name, variant, B, T, exact, iters):
    """The definition's answer (with gains) and its trace, computed once."""
    key = (name, variant, B, T, exact, iters)
    if key not in _REFS:
        c, args, kw = problem(name, variant, B, T)
        trace = []
        ref = m4q.plant_sqp_reference(*args, iters=iters, exact=exact, gains=True, trace=trace, **kw)
        for a in ref.values():
            a.setflags(write=False)
        _REFS[key] = (ref, trace)
    return _REFS[key]


def margins(trace, tol):
    """The relative margins of every decision a trace records: (best against the next candidate, J_j* < J, dec against tol J), the
    smallest of each over the trace.  Candidates whose controls equal the winner's bit for bit (the clip brought them to the same
    point) have the winner's cost bit for bit on the device as in the definition - one arithmetic on one input - and the smallest j
    wins on both sides: such a tie is no rounding decision and is left out.  So is J_j* = J of a winner whose controls are the
    iterate's bit for bit (every candidate clipped back onto it: status 2 on both sides)."""
    gap, descent, stop = np.inf, np.inf, np.inf
    for rec in trace:
        Js = np.array(rec["Js"])
        j = int(np.argmin(Js))
        others = [Js[i] for i in range(len(Js)) if i != j and not np.array_equal(rec["Us"][i], rec["Us"][j])]
        J = rec["J"]
        if others:
            gap = min(gap, (min(others) - Js[j]) / J)
        if not np.array_equal(rec["Us"][j], rec["U"]):
            descent = min(descent, abs(J - Js[j]) / J)
        if Js[j] < J:
            stop = min(stop, abs((J - Js[j]) - tol * J) / J)
    return gap, descent, stop


_CONVERGED = {}


def converged_start(name="4-2", B=3, T=6, exact=True):
    """A start from a converged U: the definition run with tol = 0 (so that only 'no candidate lowers the cost' stops a member)
    until every member has stopped that way; exact, so that the point is a minimiser of the box-constrained problem (the clipped
    mode also stops where its clipped step is no descent direction, by a margin).  Returns (c, args with U0 replaced, kw, exact)."""
    key = (name, B, T, exact)
    if key not in _CONVERGED:
        c, args, kw = problem(name, "per", 5, T)                   # (its first B members)
        args = tuple(a[:B] if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a for a in args)
        kw = dict(kw, u_prev=kw["u_prev"][:B])
        U = args[1]
        for _ in range(12):
            out = m4q.plant_sqp_reference(args[0], U, *args[2:], iters=64, exact=exact, **dict(kw, tol=0.0))
            U = out["U"]
            if np.all(out["status"] == 2):
                break
        assert np.all(out["status"] == 2), out["status"]
        U = np.ascontiguousarray(U)
        U.setflags(write=False)
        _CONVERGED[key] = (c, (args[0], U) + args[2:], kw, exact)
    return _CONVERGED[key]


# The definition's amplification at iters = 3, case by case: the largest relative change of any output (over max(1, max|output|))
# under random relative perturbations of 1e-12 of x0, U0 and the operators, over 1e-12.  Recorded by
# tests/test_plant_sqp_host.py::test_amplification_of_the_gpu_cases, which prints the table; the GPU file's iters = 3 bound is
# TOL max(1, 10 s).
AMPLIFICATION = {
    "4-1/shared-5-6/clipped": 6.7, "4-1/shared-5-6/exact": 4.6, "4-1/per-5-6/clipped": 69.2, "4-1/per-5-6/exact": 189.2,
    "4-1/shared-5-1/clipped": 2.7, "4-1/shared-5-1/exact": 0.7, "4-1/per-1-1/clipped": 0.9, "4-1/per-1-1/exact": 0.2,
    "4-1/shared-1-6/clipped": 7.7, "4-1/shared-1-6/exact": 2.5, "4-2/shared-5-6/clipped": 5004.8, "4-2/shared-5-6/exact": 1421.2,
    "4-2/per-5-6/clipped": 875.4, "4-2/per-5-6/exact": 195.5, "4-2/shared-5-1/clipped": 1.4, "4-2/shared-5-1/exact": 1.6,
    "4-2/per-1-1/clipped": 1.4, "4-2/per-1-1/exact": 1.4, "4-2/shared-1-6/clipped": 106.5, "4-2/shared-1-6/exact": 275.6,
    "9-2/shared-5-6/clipped": 6.3, "9-2/shared-5-6/exact": 2.1, "9-2/per-5-6/clipped": 17.8, "9-2/per-5-6/exact": 6.0,
    "9-2/shared-5-1/clipped": 2.0, "9-2/shared-5-1/exact": 1.7, "9-2/per-1-1/clipped": 0.6, "9-2/per-1-1/exact": 1.4,
    "9-2/shared-1-6/clipped": 12.6, "9-2/shared-1-6/exact": 9.0, "16-1/shared-5-6/clipped": 23.4, "16-1/shared-5-6/exact": 17.5,
    "16-1/per-5-6/clipped": 31.4, "16-1/per-5-6/exact": 31.5, "16-1/shared-5-1/clipped": 1.4, "16-1/shared-5-1/exact": 1.0,
    "16-1/per-1-1/clipped": 1.5, "16-1/per-1-1/exact": 0.3, "16-1/shared-1-6/clipped": 147.2, "16-1/shared-1-6/exact": 233.7,
    "16-1-process/shared-5-6/clipped": 1.2, "16-1-process/shared-5-6/exact": 5.3, "16-1-process/per-5-6/clipped": 2.8,
    "16-1-process/per-5-6/exact": 2.2, "16-1-process/shared-5-1/clipped": 0.8, "16-1-process/shared-5-1/exact": 1.3,
    "16-1-process/per-1-1/clipped": 0.7, "16-1-process/per-1-1/exact": 0.6, "16-1-process/shared-1-6/clipped": 1.2,
    "16-1-process/shared-1-6/exact": 1.1, "16-3/shared-5-6/clipped": 81.2, "16-3/shared-5-6/exact": 39.6,
    "16-3/per-5-6/clipped": 29.8, "16-3/per-5-6/exact": 13.3, "16-3/shared-5-1/clipped": 1.8, "16-3/shared-5-1/exact": 5.1,
    "16-3/per-1-1/clipped": 9.3, "16-3/per-1-1/exact": 14.9, "16-3/shared-1-6/clipped": 206.8, "16-3/shared-1-6/exact": 105.8,
    "16-3-process/shared-5-6/clipped": 6.2, "16-3-process/shared-5-6/exact": 8.7, "16-3-process/per-5-6/clipped": 6.4,
    "16-3-process/per-5-6/exact": 17.2, "16-3-process/shared-5-1/clipped": 2.7, "16-3-process/shared-5-1/exact": 3.5,
    "16-3-process/per-1-1/clipped": 0.8, "16-3-process/per-1-1/exact": 1.5, "16-3-process/shared-1-6/clipped": 6.5,
    "16-3-process/shared-1-6/exact": 3.2,
}

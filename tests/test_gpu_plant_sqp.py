"""The SQP on the plant itself in one device call (m4q_plant_sqp_batch: plant_step_kernel<PLANT, false> between the two kernels of
launch_plant_qp) against the NumPy / SciPy definition of mpc4quantum_amd/plant_sqp.py, which tests/test_plant_sqp_host.py holds to
the gradient and to its own fixed points; bit for bit against chained calls, the rollout and the one-call QP; placement; the second
trip of the grid; a converged start; refusals.  Cases, margins and the recorded amplification: tests/plant_sqp_cases.py.  Every
compiled cell of tests/test_gpu_plant_qp.py, B in {1, 5} (a ragged quad), T in {1, 6}, steps = 4, clipped and exact."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests import plant_sqp_cases as sc
from tests.test_gpu_plant_qp import TOL, _cells
from tests.test_plant_sqp_host import WHO, _Call

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
IDS = [sc.case_id(*c) for c in CASES]
FLOATS = ("X", "U", "cost", "cost_hist", "gains")
EXACT = ("alpha_hist", "n_iter", "status")


def test_the_cells_are_the_built_ones():
    assert sc.CELLS == _cells()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rel(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


_RUNS = {}


def _run(case, iters):
    """The device's answer (with gains), computed once."""
    key = case + (iters,)
    if key not in _RUNS:
        c, args, kw = sc.problem(*case[:4])
        _RUNS[key] = m4q.plant_sqp_batch(*args, iters=iters, exact=case[4], gains=True, **kw)
    return _RUNS[key]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_definition(case, iters):
    """iters = 1: the family's own bound.  iters = 3: TOL max(1, 10 s) with s the case's recorded amplification (a sampled value,
    hence the 10).  The decisions are equal exactly: none of them is a rounding decision (tests/test_plant_sqp_host.py)."""
    c, args, kw = sc.problem(*case[:4])
    ref, _ = sc.reference(*case, iters)
    out = _run(case, iters)
    s = sc.AMPLIFICATION[sc.case_id(*case)]
    bound = TOL if iters == 1 else TOL * max(1.0, 10 * s)
    errs = []
    for what in FLOATS:
        assert out[what].shape == ref[what].shape and out[what].dtype == ref[what].dtype and np.isfinite(out[what]).all(), what
        errs.append(_rel(out[what], ref[what]))
    print("%s iters=%d: X %.2e, U %.2e, cost %.2e, cost_hist %.2e, gains %.2e, each over max(1, max|ref|); bound %.1e (s = %.1f); "
          "status %s, alphas %s" % (sc.case_id(*case), iters, *errs, bound, s, out["status"], sorted(set(out["alpha_hist"].reshape(-1)))))
    for what in EXACT:
        assert out[what].dtype == ref[what].dtype and np.array_equal(out[what], ref[what]), what
    assert max(errs) <= bound
    lo, hi = sc.bounds(args, kw)
    assert np.all(out["U"] >= lo) and np.all(out["U"] <= hi)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_against_chained_calls_the_rollout_and_the_qp(case):
    c, args, kw = sc.problem(*case[:4])
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    T = U0.shape[-2]
    out = _run(case, 3)
    # three calls of one iteration, each from the controls the one before returned
    U, running = U0, np.ones(x0.shape[0], dtype=bool)
    for i in range(3):
        step = m4q.plant_sqp_batch(x0, U, *args[2:], iters=1, exact=case[4], **kw)
        U = step["U"]
        running &= step["status"] == 0
        assert np.array_equal(step["alpha_hist"][:, 0], out["alpha_hist"][:, i])
    assert np.array_equal(running, out["status"] == 0)
    for what in ("U", "X", "cost"):
        assert _bits(step[what][running], out[what][running]), what
    # the returned trajectory is the rollout's under the returned controls
    xs = m4q.plant_rollout_batch(x0, out["U"], op0, ops, ts, c.kind, u_scale=kw["u_scale"], keep="all")["xs"]
    assert _bits(xs, out["X"])
    # the gains are the one-call QP's at the returned point
    qp = m4q.plant_quad_program_batch(np.ascontiguousarray(out["X"][:, :T]), out["U"], op0, ops, ts, X_bm, U_bm, Q, R, sat, du=kw.get("du"),
                                      u_prev=kw.get("u_prev"), x_init=x0, kind=c.kind, u_scale=kw["u_scale"], exact=case[4])
    assert _bits(qp[3], out["gains"])


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("name", sc.CELLS)
def test_a_member_does_not_depend_on_its_place_nor_on_the_gains(name, exact):
    case = (name, "per", 5, 6, exact)
    c, args, kw = sc.problem(*case[:4])
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    full = _run(case, 3)
    for b in range(5):
        alone = m4q.plant_sqp_batch(x0[b:b + 1], U0[b:b + 1], op0[b], ops[b], ts, X_bm[b], U_bm[b], Q, R, sat, iters=3, exact=exact,
                                    gains=True, **dict(kw, u_prev=kw["u_prev"][b]))
        for what in FLOATS + EXACT:
            assert _bits(alone[what][0], full[what][b]), (what, b)
    less = m4q.plant_sqp_batch(*args, iters=3, exact=exact, **kw)
    assert less["gains"] is None
    for what in less:
        assert what == "gains" or _bits(less[what], full[what]), what


@pytest.mark.parametrize("name", ["4-1", "16-1-process"])
def test_the_second_trip_of_the_grid(name):
    """Five distinct members tiled to just past QUAD_WRAP members, T = 2: the step kernel's quads (and both QP kernels') are past
    their grids' wrap.  The first and last members and the members beside the wrap equal their B = 5 bits, clipped and exact."""
    c, args, kw = sc.problem(name, "per", 5, 6)
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    T = 2
    small = (x0, U0[:, :T], op0, ops, ts, X_bm[:, :T + 1], U_bm[:, :T], Q, R, sat)
    B = kv.QUAD_WRAP + 6
    assert B % kv.ROWS and B > kv.QUAD_WRAP
    tile = lambda a: np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])) if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a
    assert _bits(tile(x0)[5:10], x0)
    big = tuple(tile(a) for a in small)
    for exact in (False, True):
        want = m4q.plant_sqp_batch(*small, iters=2, exact=exact, gains=True, **kw)
        got = m4q.plant_sqp_batch(*big, iters=2, exact=exact, gains=True, **dict(kw, u_prev=tile(kw["u_prev"])))
        assert want["n_iter"].max() == 2
        for b in (0, 1, kv.QUAD_WRAP - 1, kv.QUAD_WRAP, kv.QUAD_WRAP + 1, B - 2, B - 1):
            for what in FLOATS + EXACT:
                assert _bits(got[what][b], want[what][b % 5]), (what, b, exact)


def test_the_converged_start():
    """From a converged U the only decrease left is rounding: the device stops with status 1 or 2 as the definition does (which of
    the two is a rounding decision, ~1e-16 of the cost against tol = 1e-9), after at most one accepted step that changes the cost by
    no more than tol, and a member that found no descent keeps its controls bit for bit."""
    c, args, kw, exact = sc.converged_start()
    ref = m4q.plant_sqp_reference(*args, iters=3, exact=exact, **kw)
    out = m4q.plant_sqp_batch(*args, iters=3, exact=exact, **kw)
    U0 = args[1]
    for res in (ref, out):
        assert np.all((res["status"] == 1) | (res["status"] == 2)) and np.all(res["n_iter"] <= 1)
        assert np.array_equal(res["n_iter"] == 0, res["status"] == 2)
    print("converged start: status %s (definition %s), relative decrease %s" % (out["status"], ref["status"],
                                                                                (out["cost_hist"][:, 0] - out["cost"]) / out["cost"]))
    same = out["status"] == 2
    assert _bits(out["U"][same], U0[same])
    assert np.all(out["cost_hist"][:, 0] - out["cost"] <= 1e-3 * kw["tol"] * out["cost"])
    # the cost is the definition's either way; the controls where the two took the same decision (a step accepted at the flat
    # bottom moves U by what the QP returns there, ~1e-9, for a change of ~1e-16 in the cost)
    assert _rel(out["cost"], ref["cost"]) <= TOL
    agree = out["status"] == ref["status"]
    assert agree.any()
    assert _rel(out["U"][agree], ref["U"][agree]) <= TOL and _rel(out["X"][agree], ref["X"][agree]) <= TOL


def test_the_experiment_wrappers_return_the_module_function_s_arrays():
    c, args, kw = sc.problem("9-2", "shared", 5, 6)
    want = _run(("9-2", "shared", 5, 6, True), 3)
    got = m4q.QExperiment(c.op0, list(c.ops)).sqp_batch(args[0], args[1], args[4], *args[5:], iters=3, steps=sc.STEPS, tol=sc.TOL_SQP,
                                                        u_scale=kw["u_scale"], exact=True, gains=True)
    assert all(_bits(got[k], want[k]) for k in want)
    c, args, kw = sc.problem("9-2", "per", 5, 6)
    # (per-member op0 with the experiment's own control operators)
    want = m4q.plant_sqp_batch(args[0], args[1], args[2], c.ops, *args[4:], iters=3, **kw)
    got = m4q.QExperiment(c.op0, list(c.ops)).sqp_batch(args[0], args[1], args[4], *args[5:], iters=3, steps=sc.STEPS, tol=sc.TOL_SQP,
                                                        du=kw["du"], u_prev=kw["u_prev"], op0=args[2])
    assert got["gains"] is None and all(_bits(got[k], want[k]) for k in want if k != "gains")
    c, args, kw = sc.problem("16-1-process", "shared", 5, 6)
    want = _run(("16-1-process", "shared", 5, 6, False), 3)
    got = m4q.QSynthesis(c.op0, list(c.ops)).sqp_batch(args[0], args[1], args[4], *args[5:], iters=3, steps=sc.STEPS, tol=sc.TOL_SQP,
                                                       u_scale=kw["u_scale"], gains=True)
    assert all(_bits(got[k], want[k]) for k in want)


def test_the_generator_plant_and_the_plant_only_shape_are_refused():
    L = _lib.lib()
    assert _Call(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"generator plant has no kernel" in L.m4q_last_error()
    assert _Call(n=16, m=2, k=4)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"plant-only" in L.m4q_last_error()
    c = gc.plant_case("16-2")
    x0, U = np.zeros((2, 16), complex), np.zeros((3, 2))
    with pytest.raises(_lib.M4qError, match="plant-only"):
        m4q.plant_sqp_batch(x0, U, c.op0, c.ops, c.dt, np.zeros((4, 16)), U, np.eye(16), np.eye(2), 1.0)
    with pytest.raises(ValueError, match="generator plant"):
        m4q.plant_sqp_batch(np.zeros((2, 9), complex), U, np.eye(9), np.stack([np.eye(9)] * 2), 0.1, np.zeros((4, 9)), U, np.eye(9),
                            np.eye(2), 1.0, kind=_lib.PLANT_GENERATOR)

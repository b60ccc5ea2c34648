"""The iLQR on the plant itself in one device call (m4q_plant_ilqr_batch: plant_step_kernel<PLANT, true> between the two kernels of
launch_plant_qp) against the NumPy / SciPy definition of mpc4quantum_amd/plant_ilqr.py, which tests/test_plant_ilqr_host.py holds to
itself and to its neighbours; bit for bit against chained calls (the in-place hand-over of the iterate), the rollout and the
one-call QP; placement; against the stored law of plant_feedback_batch and against plant_sqp_batch where the two must agree; the
second trip of the grid; a converged start; a member whose first cost is not finite; refusals.  Cases, margins and the recorded
amplification: tests/plant_ilqr_cases.py.  Every compiled cell of tests/test_gpu_plant_qp.py, B in {1, 5} (a ragged quad), T in
{1, 6}, steps = 4, clipped and exact."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests import plant_ilqr_cases as ic
from tests.test_gpu_plant_qp import TOL, _cells
from tests.test_plant_ilqr_host import WHO, _Call, stored_law

pytestmark = pytest.mark.gpu

CASES = ic.all_cases()
IDS = [ic.case_id(*c) for c in CASES]
FLOATS = ("X", "U", "cost", "cost_hist", "gains")
EXACT = ("alpha_hist", "n_iter", "status")


def test_the_cells_are_the_built_ones():
    """The kernel is built where launch_plant_qp is: the cells of tests/test_gpu_plant_qp.py, Hamiltonian and process plants."""
    assert ic.CELLS == _cells()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rel(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def bound(case, iters):
    """TOL max(1, 10 s): s the case's recorded amplification at that iteration count (a sampled value, hence the 10)."""
    return TOL * max(1.0, 10 * ic.AMPLIFICATION[ic.case_id(*case)][0 if iters == 1 else 1])


_RUNS = {}


def _run(case, iters):
    """The device's answer (with gains), computed once."""
    key = case + (iters,)
    if key not in _RUNS:
        c, args, kw = ic.problem(*case[:4])
        _RUNS[key] = m4q.plant_ilqr_batch(*args, iters=iters, exact=case[4], gains=True, **kw)
    return _RUNS[key]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_definition(case, iters):
    """The decisions are equal exactly - none of them is a rounding decision (tests/test_plant_ilqr_host.py) - and every member is
    compared."""
    c, args, kw = ic.problem(*case[:4])
    ref, _ = ic.reference(*case, iters)
    out = _run(case, iters)
    assert sorted(out) == sorted(ref)
    errs = []
    for what in FLOATS:
        assert out[what].shape == ref[what].shape and out[what].dtype == ref[what].dtype and np.isfinite(out[what]).all(), what
        errs.append(_rel(out[what], ref[what]))
    print("%s iters=%d: X %.2e, U %.2e, cost %.2e, cost_hist %.2e, gains %.2e, each over max(1, max|ref|); bound %.1e; "
          "status %s, alphas %s" % (ic.case_id(*case), iters, *errs, bound(case, iters), out["status"],
                                    sorted(set(out["alpha_hist"].reshape(-1)))))
    for what in EXACT:
        assert out[what].dtype == ref[what].dtype and np.array_equal(out[what], ref[what]), what
    assert max(errs) <= bound(case, iters)
    lo, hi = ic.bounds(args, kw)
    assert np.all(out["U"] >= lo) and np.all(out["U"] <= hi)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_against_chained_calls_the_rollout_and_the_qp(case):
    c, args, kw = ic.problem(*case[:4])
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    T = U0.shape[-2]
    out = _run(case, 3)
    # three calls of one iteration, each from the controls the one before returned: the iterate the step kernel hands over in place
    # (X_lin, U) is what a fresh call rolls out of those controls
    U, running = U0, np.ones(x0.shape[0], dtype=bool)
    for i in range(3):
        step = m4q.plant_ilqr_batch(x0, U, *args[2:], iters=1, exact=case[4], **kw)
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
@pytest.mark.parametrize("name", ic.CELLS)
def test_a_member_does_not_depend_on_its_place_nor_on_the_gains(name, exact):
    case = (name, "per", 5, 6, exact)
    c, args, kw = ic.problem(*case[:4])
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    full = _run(case, 3)
    for b in range(5):
        alone = m4q.plant_ilqr_batch(x0[b:b + 1], U0[b:b + 1], op0[b], ops[b], ts, X_bm[b], U_bm[b], Q, R, sat, iters=3, exact=exact,
                                     gains=True, **dict(kw, u_prev=kw["u_prev"][b]))
        for what in FLOATS + EXACT:
            assert _bits(alone[what][0], full[what][b]), (what, b)
    less = m4q.plant_ilqr_batch(*args, iters=3, exact=exact, **kw)
    assert less["gains"] is None
    for what in less:
        assert what == "gains" or _bits(less[what], full[what]), what


@pytest.mark.parametrize("B,T", [(5, 6), (5, 1), (1, 6)])
@pytest.mark.parametrize("name", ic.CELLS)
def test_a_full_step_against_the_stored_law(name, B, T):
    """The "shared" runs (no band), clipped, iters = 1, steps = 1: where the step was accepted, U and X are plant_feedback_batch's
    under the law of the QP at the initial roll - within the bound of the first test at iters = 1, not bit for bit (the two
    associate the control's terms differently)."""
    case = (name, "shared", B, T, False)
    c, args, kw = ic.problem(*case[:4])
    out = m4q.plant_ilqr_batch(*args, iters=1, exact=False, **dict(kw, steps=1))
    fb = m4q.plant_feedback_batch(args[0], stored_law(c, args, kw), args[2], args[3], args[4], kind=c.kind, u_scale=kw["u_scale"],
                                  controls=True)
    took = out["n_iter"] == 1
    assert took.any()
    eu, ex = _rel(out["U"][took], fb["us"][took]), _rel(out["X"][took], fb["xs"][took])
    print("%s: %d of %d accepted, U %.2e, X %.2e; bound %.1e" % (ic.case_id(*case), took.sum(), B, eu, ex, bound(case, 1)))
    assert max(eu, ex) <= bound(case, 1)


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("variant,B", [("shared", 5), ("per", 1)])
@pytest.mark.parametrize("name", ic.CELLS)
def test_at_one_step_and_a_full_step_length_it_is_the_sqp(name, variant, B, exact):
    """T = 1, steps = 1: nothing to feed back, and the candidate is the SQP's up to the rounding of one sum
    (tests/test_plant_ilqr_host.py holds the two definitions together)."""
    case = (name, variant, B, 1, exact)
    c, args, kw = ic.problem(*case[:4])
    kw = dict(kw, steps=1)
    got = m4q.plant_ilqr_batch(*args, iters=1, exact=exact, gains=True, **kw)
    want = m4q.plant_sqp_batch(*args, iters=1, exact=exact, gains=True, **kw)
    for what in EXACT:
        assert np.array_equal(got[what], want[what]), what
    errs = [_rel(got[what], want[what]) for what in FLOATS]
    print("%s: %s; bound %.1e" % (ic.case_id(*case), " ".join("%.1e" % e for e in errs), bound(case, 1)))
    assert max(errs) <= bound(case, 1)


@pytest.mark.parametrize("name", ["4-1", "16-1-process"])
def test_the_second_trip_of_the_grid(name):
    """Five distinct members tiled to just past QUAD_WRAP members, T = 2: the step kernel's quads (and both QP kernels') are past
    their grids' wrap.  The first and last members and the members beside the wrap equal their B = 5 bits, clipped and exact."""
    c, args, kw = ic.problem(name, "per", 5, 6)
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    T = 2
    small = (x0, U0[:, :T], op0, ops, ts, X_bm[:, :T + 1], U_bm[:, :T], Q, R, sat)
    B = kv.QUAD_WRAP + 6
    assert B % kv.ROWS and B > kv.QUAD_WRAP
    tile = lambda a: np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])) if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a
    assert _bits(tile(x0)[5:10], x0)
    big = tuple(tile(a) for a in small)
    for exact in (False, True):
        want = m4q.plant_ilqr_batch(*small, iters=2, exact=exact, gains=True, **kw)
        got = m4q.plant_ilqr_batch(*big, iters=2, exact=exact, gains=True, **dict(kw, u_prev=tile(kw["u_prev"])))
        assert want["n_iter"].max() == 2
        for b in (0, 1, kv.QUAD_WRAP - 1, kv.QUAD_WRAP, kv.QUAD_WRAP + 1, B - 2, B - 1):
            for what in FLOATS + EXACT:
                assert _bits(got[what][b], want[what][b % 5]), (what, b, exact)


@pytest.mark.parametrize("B,box", [(3, 1.0), (5, ic.NARROW)], ids=["interior", "narrow-box"])
def test_the_converged_start(B, box):
    """From the definition's own converged point (exact) no member moves.  A member every one of whose controls the QP pins
    (the narrow box has four of five) has the iterate for every candidate: status 2 is required of it.  For any other the
    decrease a candidate can still make is rounding (~1e-16 of the cost) against tol = 1e-9: it stops with status 2, or, where the
    device's rounding does find such a decrease, with status 1 after one step that changes the cost by no more than tol.  With
    status 2, U and X are the start's and its rollout's bit for bit; after such a step they are within
    plant_ilqr_cases.move_bounds of them.  (MI355X: the interior start stops [1, 1, 1] after steps worth 1.2 - 1.9e-16 of J that move
    U by at most 1.3e-8; the narrow box [2, 1, 2, 2, 2], its free member after a step worth 3.3e-13 of J that moves U by 6.2e-7.)"""
    c, args, kw, exact = ic.converged_start(B=B, box=box)
    x0, U0, op0, ops, ts = args[:5]
    ref = m4q.plant_ilqr_reference(*args, iters=3, exact=exact, **kw)
    out = m4q.plant_ilqr_batch(*args, iters=3, exact=exact, **kw)
    X0 = m4q.plant_rollout_batch(x0, U0, op0, ops, ts, c.kind, u_scale=kw["u_scale"], keep="all")["xs"]
    held = ic.held_members(args, kw, exact)
    assert held.sum() == (0 if box == 1.0 else 4)
    assert np.all(ref["status"] == 2) and np.all(ref["n_iter"] == 0) and _bits(ref["U"], U0)
    assert np.all((out["status"] == 1) | (out["status"] == 2)) and np.all(out["n_iter"] <= 1)
    assert np.array_equal(out["n_iter"] == 0, out["status"] == 2)
    dU, dX = ic.move_bounds(args, kw, ref["cost"])
    eU, eX = np.abs(out["U"] - U0).max(axis=(1, 2)), np.abs(out["X"] - X0).max(axis=(1, 2))
    print("converged start (%s): status %s, held %s, relative decrease %s, max|U - U0| %s (bound %s), max|X - X(U0)| %s (bound %s)" % (
        "interior" if box == 1.0 else "narrow box", out["status"], held, (out["cost_hist"][:, 0] - out["cost"]) / out["cost"], eU, dU, eX, dX))
    same = out["status"] == 2
    assert np.all(same[held])
    assert _bits(out["U"][same], U0[same]) and _bits(out["X"][same], X0[same])
    assert np.all(eU <= dU) and np.all(eX <= dX)
    assert np.all(out["cost_hist"][:, 0] - out["cost"] <= 1e-3 * kw["tol"] * out["cost"])
    assert _rel(out["cost"], ref["cost"]) <= TOL
    lo, hi = ic.bounds(args, kw)
    assert np.all(out["U"] >= lo) and np.all(out["U"] <= hi)


def test_a_first_cost_that_is_not_finite():
    """Member 1 of five starts from a NaN state: status 3, no iteration, its first cost in every history entry, and the other
    members - three of them in its quad - have the bits they have without it.  (Clipped: the QP of every iteration runs on every
    member, and what the exact solver makes of a NaN member is its own matter.)"""
    case = ("9-2", "per", 5, 6, False)
    c, args, kw = ic.problem(*case[:4])
    x0 = np.array(args[0])
    x0[1] = np.nan
    want = _run(case, 3)
    got = m4q.plant_ilqr_batch(x0, *args[1:], iters=3, exact=False, gains=True, **kw)
    ref = m4q.plant_ilqr_reference(x0, *args[1:], iters=3, exact=False, **kw)
    assert got["status"][1] == ref["status"][1] == 3 and got["n_iter"][1] == 0 and np.all(got["alpha_hist"][1] == 0)
    assert np.isnan(got["cost"][1]) and np.isnan(got["cost_hist"][1]).all()
    lo, hi = ic.bounds(args, kw)
    assert _bits(got["U"][1], np.minimum(np.maximum(args[1][1], lo[1]), hi[1]))
    others = [0, 2, 3, 4]
    for what in FLOATS + EXACT:
        assert _bits(got[what][others], want[what][others]), what


def test_the_experiment_wrappers_return_the_module_function_s_arrays():
    c, args, kw = ic.problem("9-2", "shared", 5, 6)
    want = _run(("9-2", "shared", 5, 6, True), 3)
    got = m4q.QExperiment(c.op0, list(c.ops)).ilqr_batch(args[0], args[1], args[4], *args[5:], iters=3, steps=ic.STEPS, tol=ic.TOL_SQP,
                                                         u_scale=kw["u_scale"], exact=True, gains=True)
    assert all(_bits(got[k], want[k]) for k in want)
    c, args, kw = ic.problem("16-1-process", "shared", 5, 6)
    want = _run(("16-1-process", "shared", 5, 6, False), 3)
    got = m4q.QSynthesis(c.op0, list(c.ops)).ilqr_batch(args[0], args[1], args[4], *args[5:], iters=3, steps=ic.STEPS, tol=ic.TOL_SQP,
                                                        u_scale=kw["u_scale"], gains=True)
    assert all(_bits(got[k], want[k]) for k in want)


def test_the_generator_plant_and_the_plant_only_shape_are_refused():
    L = _lib.lib()
    assert _Call(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"generator plant has no kernel" in L.m4q_last_error()
    assert _Call(n=16, m=2, k=4)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"plant-only" in L.m4q_last_error()
    assert _Call()(iters=0) == _lib.E_BADARG and WHO in L.m4q_last_error() and b"iters" in L.m4q_last_error()
    assert _Call()(steps=9) == _lib.E_BADARG and WHO in L.m4q_last_error() and b"steps" in L.m4q_last_error()
    assert _Call()(x0=None) == _lib.E_BADARG and WHO in L.m4q_last_error() and b"x0" in L.m4q_last_error()
    c = gc.plant_case("16-2")
    x0, U = np.zeros((2, 16), complex), np.zeros((3, 2))
    with pytest.raises(_lib.M4qError, match="plant-only"):
        m4q.plant_ilqr_batch(x0, U, c.op0, c.ops, c.dt, np.zeros((4, 16)), U, np.eye(16), np.eye(2), 1.0)
    with pytest.raises(ValueError, match="generator plant"):
        m4q.plant_ilqr_batch(np.zeros((2, 9), complex), U, np.eye(9), np.stack([np.eye(9)] * 2), 0.1, np.zeros((4, 9)), U, np.eye(9),
                             np.eye(2), 1.0, kind=_lib.PLANT_GENERATOR)

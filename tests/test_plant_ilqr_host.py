"""The iLQR on the plant itself (m4q_plant_ilqr_batch) without a GPU: the NumPy / SciPy definition of mpc4quantum_amd/plant_ilqr.py
held to itself and to its neighbours - a monotone descent, the SQP's answer where there is no later state to feed back, the stored
law of feedback.py at a full step, pinned controls on their bounds, its own converged points as fixed points - the decision margins
and the amplification of every case tests/test_gpu_plant_ilqr.py runs, every refusal of the C entry point (all come back before a
device is asked for), and the prototype against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, plant_ilqr, plant_sqp
from mpc4quantum_amd.feedback import _plant_step
from tests import plant_ilqr_cases as ic
from tests import test_plant_sqp_host as sqp_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"m4q_plant_ilqr_batch"
CASES = ic.all_cases()
IDS = [ic.case_id(*c) for c in CASES]
ROUNDING = 1e-12                                                   # "to rounding": see the tests that use it
_rel = sqp_host._rel


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cost_never_rises_and_is_the_cost_of_the_returned_controls(case):
    name, variant, B, T, exact = case
    c, args, kw = ic.problem(name, variant, B, T)
    ref, trace = ic.reference(*case, 3)
    assert np.all(np.diff(ref["cost_hist"], axis=1) <= 0)
    assert np.array_equal(ref["cost_hist"][:, -1], ref["cost"])
    lo, hi = ic.bounds(args, kw)
    assert np.all(ref["U"] >= lo) and np.all(ref["U"] <= hi)
    assert ref["cost_hist"][:, -1].sum() < ref["cost_hist"][:, 0].sum()
    # the accepted (U, X, J) are the candidate's: the trajectory is the plant's under the returned controls, bit for bit
    for b in range(B):
        x0, s, op0, ops, dts, Xb, Ub = sqp_host._member(args, kw, b)
        x = x0
        for t in range(T):
            assert np.array_equal(ref["X"][b, t], x)
            x = _plant_step(c.kind, x, s * ref["U"][b, t], op0, ops, dts[t])
        assert np.array_equal(ref["X"][b, T], x)


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("variant,B", [("shared", 5), ("per", 1)])
@pytest.mark.parametrize("name", ic.CELLS)
def test_at_one_step_and_a_full_step_length_it_is_the_sqp(name, variant, B, exact):
    """T = 1: x_0 is the iterate's, there is nothing to feed back, and at a = 1 the candidate is clip(Ubar + (pi - Ubar)) against the
    SQP's clip(Ubar + (clip(pi) - Ubar)): the same control up to the two roundings of the sum (a few ulp of the bound), whose
    effect on x_1 and on the cost is of the same order - ROUNDING is a thousand times that.  One iteration, so that nothing grows."""
    c, args, kw = ic.problem(name, variant, B, 1)
    kw = dict(kw, steps=1)
    got = m4q.plant_ilqr_reference(*args, iters=1, exact=exact, gains=True, **kw)
    want = m4q.plant_sqp_reference(*args, iters=1, exact=exact, gains=True, **kw)
    for what in ("alpha_hist", "n_iter", "status"):
        assert np.array_equal(got[what], want[what]), what
    errs = [_rel(got[what], want[what]) for what in ("X", "U", "cost", "cost_hist", "gains")]
    print("%s/%s-%d-1/%s: %s" % (name, variant, B, "exact" if exact else "clipped", " ".join("%.1e" % e for e in errs)))
    assert max(errs[:4]) <= ROUNDING
    assert errs[4] <= 1e3 * ROUNDING                               # (the gains: one more linearisation and QP behind those controls)


def _initial_roll(c, args, kw):
    """(U, X) of the initial roll of a problem: clip(U0) and the plant's trajectory under it."""
    x0, U0 = args[0], args[1]
    B, (T, m) = x0.shape[0], U0.shape[-2:]
    lo, hi = ic.bounds(args, kw)
    U = np.minimum(np.maximum(np.broadcast_to(U0, (B, T, m)), lo), hi)
    X = np.empty((B, T + 1, x0.shape[1]), dtype=complex)
    for b in range(B):
        xb, s, op0, ops, dts = sqp_host._member(args, kw, b)[:5]
        X[b, 0] = xb
        for t in range(T):
            X[b, t + 1] = _plant_step(c.kind, X[b, t], s * U[b, t], op0, ops, dts[t])
    return U, X


def stored_law(c, args, kw):
    """The law of the QP at the initial roll of a problem without a band, as a per-member FeedbackLaw around the targets."""
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    B, (T, m) = x0.shape[0], U0.shape[-2:]
    U, X = _initial_roll(c, args, kw)
    K = m4q.plant_quad_program_reference(X[:, :T], U, op0, ops, ts, X_bm, U_bm, Q, R, sat, x_init=x0, kind=c.kind,
                                         u_scale=kw["u_scale"])[3]
    return m4q.FeedbackLaw(K, np.broadcast_to(X_bm, (B,) + X_bm.shape[-2:]), np.broadcast_to(U_bm, (B, T, m)), sat)


@pytest.mark.parametrize("B,T", [(5, 6), (5, 1), (1, 6)])
@pytest.mark.parametrize("name", ic.CELLS)
def test_a_full_step_is_the_stored_law_on_the_plant(name, B, T):
    """iters = 1, steps = 1, clipped, no band: an accepted trajectory is plant_feedback_reference's under the QP's law.  The two
    associate differently (Ubar + (pi(Xbar) - Ubar) + K (x - Xbar) against K (x - xb) + k + ub): a few roundings of |K| |x| per
    step, fed through at most six steps of a stabilised loop."""
    c, args, kw = ic.problem(name, "shared", B, T)
    assert kw.get("du") is None
    out = m4q.plant_ilqr_reference(*args, iters=1, exact=False, **dict(kw, steps=1))
    fb = m4q.plant_feedback_reference(args[0], stored_law(c, args, kw), args[2], args[3], args[4], kind=c.kind, u_scale=kw["u_scale"])
    took = out["n_iter"] == 1
    assert took.any()
    eu, ex = _rel(out["U"][took], fb["us"][took]), _rel(out["X"][took], fb["xs"][took])
    print("%s/shared-%d-%d: %d of %d accepted, U %.1e, X %.1e" % (name, B, T, took.sum(), B, eu, ex))
    assert max(eu, ex) <= ROUNDING


PINNING = [("16-3-process", "shared", 5, 6), ("4-2", "per", 5, 6)]   # runs whose QPs do leave controls on a bound


@pytest.mark.parametrize("case", [c for c in CASES if c[4] and c[3] == 6], ids=lambda c: ic.case_id(*c))
def test_a_pinned_control_of_the_full_step_sits_on_its_bound(case):
    c, args, kw = ic.problem(*case[:4])
    lo, hi = ic.bounds(args, kw)
    _, trace = ic.reference(*case, 3)
    n_pinned = 0
    for rec in trace:
        b = rec["b"]
        pinned = (rec["U_qp"] >= hi[b]) | (rec["U_qp"] <= lo[b])
        n_pinned += int(pinned.sum())
        # Ubar + (U_qp - Ubar): two roundings of numbers inside the box, then the clip
        assert np.all(np.abs(rec["Us"][0][pinned] - rec["U_qp"][pinned]) <= 4 * np.finfo(float).eps * args[9])
        # ... and it takes no feedback: it is the SQP's control at every step length
        for j, Uj in enumerate(rec["Us"]):
            line = np.minimum(np.maximum(rec["U"] + 0.5 ** j * (rec["U_qp"] - rec["U"]), lo[b]), hi[b])
            assert np.array_equal(Uj[pinned], line[pinned])
    print("%s: %d pinned controls over %d records" % (ic.case_id(*case), n_pinned, len(trace)))
    if case[:4] in PINNING:
        assert n_pinned > 0


def test_its_own_converged_point_is_a_fixed_point():
    """The restart repeats the arithmetic of the iteration that found no descent: status 2 at once, U unchanged bit for bit."""
    c, args, kw, exact = ic.converged_start()
    out = m4q.plant_ilqr_reference(*args, iters=3, exact=exact, **kw)
    assert np.all(out["status"] == plant_sqp.STATUS_NO_DESCENT) and np.all(out["n_iter"] == 0)
    assert np.array_equal(out["U"], args[1])
    assert np.all(out["alpha_hist"] == 0) and np.all(out["cost_hist"] == out["cost"][:, None])


def test_in_a_narrow_box_a_pinned_member_s_candidates_are_the_iterate():
    """The converged start of the GPU file's second case: a fixed point again; four of its five members have every control pinned
    and so every candidate the iterate, with the iterate's cost, bit for bit; the fifth has a free control.  The interior start
    has no such member.  How far an accepted rounding step may move either start (move_bounds) is of the order of sqrt(epsilon)."""
    c, args, kw, exact = ic.converged_start(B=5, box=ic.NARROW)
    trace = []
    out = m4q.plant_ilqr_reference(*args, iters=3, exact=exact, trace=trace, **kw)
    assert np.all(out["status"] == plant_sqp.STATUS_NO_DESCENT) and np.all(out["n_iter"] == 0) and np.array_equal(out["U"], args[1])
    held = ic.held_members(args, kw, exact)
    lo, hi = ic.bounds(args, kw)
    on = ((args[1] == lo) | (args[1] == hi)).reshape(5, -1).sum(1)
    print("narrow box: held %s, controls on a bound %s of %d" % (held, on, args[1][0].size))
    assert held.sum() == 4 and np.all(on[held] == args[1][0].size) and np.all(on[~held] < args[1][0].size)
    for rec in trace:
        assert all(J == rec["J"] for J in rec["Js"]) == held[rec["b"]]
    start = ic.converged_start()
    assert not ic.held_members(*start[1:]).any()
    for cs, cost in ((start, None), ((c, args, kw, exact), out["cost"])):
        if cost is None:
            cost = m4q.plant_ilqr_reference(*cs[1], iters=1, exact=cs[3], **cs[2])["cost"]
        dU, dX = ic.move_bounds(cs[1], cs[2], cost)
        print("move bounds: U %s, X %s" % (dU, dX))
        assert np.all(dU < 1e3 * np.sqrt(np.finfo(float).eps)) and np.all(dX < 50 * dU)


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
def test_gains_are_the_qp_s_at_the_returned_point(exact):
    c, args, kw = ic.problem("9-2", "per", 5, 6)
    ref, _ = ic.reference("9-2", "per", 5, 6, exact, 3)
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    want = m4q.plant_quad_program_reference(ref["X"][:, :6], ref["U"], op0, ops, ts, X_bm, U_bm, Q, R, sat, du=kw["du"], u_prev=kw["u_prev"],
                                            x_init=x0, kind=c.kind, exact=exact)[3]
    assert np.array_equal(ref["gains"], want)
    less = m4q.plant_ilqr_reference(*args, iters=3, exact=exact, **kw)
    assert less["gains"] is None and all(np.array_equal(less[k], ref[k]) for k in less if k != "gains")


def test_the_seed_shifts_are_this_file_s_own():
    """The shifted run is another draw than the SQP's and every other run is the SQP's object; this file's copy of the draw gives
    the SQP's problems bit for bit at the SQP's shifts (a shifted and an unshifted run of either variant)."""
    from tests import plant_sqp_cases as sc
    for key in ic.SEED_SHIFT:
        mine, theirs = ic.problem(*key), sc.problem(*key)
        assert mine is not theirs and not np.array_equal(mine[1][0], theirs[1][0])
        assert ic.problem(*key) is mine and sc.problem(*key) is theirs
    assert ic.problem("9-2", "per", 5, 6) is sc.problem("9-2", "per", 5, 6)
    for key in [("4-1", "shared", 5, 1), ("4-1", "per", 1, 1), ("4-2", "shared", 5, 1), ("9-2", "per", 5, 6), ("16-3-process", "shared", 1, 6)]:
        (c, args, kw), (c2, args2, kw2) = ic.draw(*key, sc.SEED_SHIFT.get(key, 0)), sc.problem(*key)
        assert c is c2 and sorted(kw) == sorted(kw2)
        for a, b in list(zip(args, args2)) + [(kw[k], kw2[k]) for k in kw]:
            assert type(a) is type(b) and np.array_equal(a, b)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decision_margins_of_the_gpu_cases(case):
    """No decision of the definition in a GPU case is a rounding decision, at either iteration count: every member is compared on
    the device.  A shifted run took the FIRST seed that passes."""
    ref, trace = ic.reference(*case, 3)
    gap, descent, stop = ic.margins(trace, ic.TOL_SQP)
    print("%s: best against the next candidate %.2e, J_j* < J by %.2e, dec against tol J %.2e (relative to J); alphas %s"
          % (ic.case_id(*case), gap, descent, stop, sorted(set(ref["alpha_hist"].reshape(-1)))))
    assert min(gap, descent, stop) >= ic.MARGIN
    assert np.all((ref["status"] == plant_sqp.STATUS_ITERS) == (ref["n_iter"] == 3))
    assert np.all((ref["status"] == plant_sqp.STATUS_ITERS) | (ref["status"] == plant_sqp.STATUS_NO_DESCENT))
    one, trace1 = ic.reference(*case[:5], 1)
    assert min(ic.margins(trace1, ic.TOL_SQP)) >= ic.MARGIN
    assert np.array_equal(one["U"], np.stack([rec["Us"][int(np.argmin(rec["Js"]))] for rec in trace if rec["i"] == 0]))


@pytest.mark.parametrize("key", sorted(ic.SEED_SHIFT))
def test_a_shifted_run_took_the_first_seed_that_passes(key, monkeypatch):
    for shift in range(ic.SEED_SHIFT[key]):
        monkeypatch.setitem(ic.SEED_SHIFT, key, shift)
        monkeypatch.setattr(ic, "_PROBLEMS", {})
        c, args, kw = ic.problem(*key)
        worst = np.inf
        for exact in (False, True):
            for iters in (1, 3):
                trace = []
                m4q.plant_ilqr_reference(*args, iters=iters, exact=exact, trace=trace, **kw)
                worst = min(worst, *ic.margins(trace, ic.TOL_SQP))
        print("%s shift %d: smallest margin %.2e" % (key, shift, worst))
        assert worst < ic.MARGIN


def _perturbed(rng, a):
    return a * (1 + ic.EPS * rng.uniform(-1, 1, a.shape))


def amplification(case, iters):
    name, variant, B, T, exact = case
    c, args, kw = ic.problem(name, variant, B, T)
    ref, _ = ic.reference(*case, iters)
    rng = np.random.default_rng(7500 + CASES.index(case))
    x0, U0, op0, ops = (_perturbed(rng, a) for a in args[:4])
    out = m4q.plant_ilqr_reference(x0, U0, op0, ops, *args[4:], iters=iters, exact=exact, gains=True, **kw)
    assert np.array_equal(out["alpha_hist"], ref["alpha_hist"]) and np.array_equal(out["status"], ref["status"])
    return max(_rel(out[k], ref[k]) for k in ("X", "U", "cost", "cost_hist", "gains")) / ic.EPS


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_amplification_of_the_gpu_cases(case):
    """The record of tests/plant_ilqr_cases.py: AMPLIFICATION is what this test computes (same seeds), at iters 1 and 3."""
    s = tuple(amplification(case, iters) for iters in (1, 3))
    print('    "%s": (%.1f, %.1f),' % (ic.case_id(*case), *s))
    assert np.isfinite(s).all()
    recorded = ic.AMPLIFICATION[ic.case_id(*case)]
    for got, rec in zip(s, recorded):
        assert got <= 10 * max(1.0, rec)                           # (the record is of this computation, up to the platform's expm)


# ---------------------------------------------------------------- the C ABI
class _Call(sqp_host._Call):
    """One valid m4q_plant_ilqr_batch call on host buffers of the right sizes: the SQP's, whose arguments these are."""

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_ilqr_batch(*[v[k] for k in self.ORDER])


@pytest.mark.parametrize("change,word", sqp_host.BAD, ids=[str(c) for c, _ in sqp_host.BAD])
def test_refuses_bad_arguments(change, word):
    assert _Call()(**change) == _lib.E_BADARG
    msg = _lib.lib().m4q_last_error()
    assert WHO in msg and word in msg


def test_refuses_what_has_no_kernel():
    L = _lib.lib()
    for call, word in ((_Call(n=25, k=5), b"no kernel"), (_Call(n=9, m=3), b"no kernel"), (_Call(n=8, m=2, k=2), b"not a square"),
                       (_Call(n=9, kind=_lib.PLANT_GENERATOR, k=9), b"generator plant has no kernel"),
                       (_Call(n=16, m=2, k=4), b"plant-only")):
        assert call() == _lib.E_UNSUPPORTED
        assert WHO in L.m4q_last_error() and word in L.m4q_last_error()
    call = _Call(n=16, m=1, k=4)
    assert call(B=4_000_000, T=3, flags=_lib.QP_EXACT_BOX) == _lib.E_BADARG
    assert WHO in L.m4q_last_error() and b"4 GiB" in L.m4q_last_error()


def test_valid_calls_reach_the_device_check():
    if _lib.device_count() > 0:
        return                                                    # (with a device these calls run: tests/test_gpu_plant_ilqr.py)
    for call in (_Call(), _Call(n=4, m=1, k=2), _Call(n=16, m=3, k=4), _Call(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2), _Call(iters=64)):
        B, m = call.v["B"], call.v["m"]
        assert call() == _lib.E_NODEVICE
        assert call(flags=_lib.QP_EXACT_BOX) == _lib.E_NODEVICE
        assert call(flags=_lib.QP_DU_BAND, du=0.5, u_prev=call._b("up", B * m)) == _lib.E_NODEVICE
        assert call(u_scale=call._b("sc", B * m), gains=call._b("g", 1), tol=0.0, steps=1) == _lib.E_NODEVICE
        assert call(steps=8) == _lib.E_NODEVICE


def test_prototype_agrees_with_the_header():
    header = open(os.path.join(ROOT, "include", "m4q.h")).read()
    params = lambda name: [" ".join(p.split()) for p in re.search(r"M4Q_API int %s\((.*?)\);" % name, header, re.S).group(1).split(",")]
    mine = params("m4q_plant_ilqr_batch")
    assert mine == params("m4q_plant_sqp_batch") and len(mine) == 33           # the SQP's arguments, in its order
    kinds = {"int32_t": _lib._i32, "double": ctypes.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int32_t*": _lib._ip}
    want = [kinds[p.rsplit(" ", 1)[0]] for p in mine]
    restype, argtypes = _lib.PROTOTYPES["m4q_plant_ilqr_batch"]
    assert restype is ctypes.c_int and len(argtypes) == len(want)
    assert all(a is w for a, w in zip(argtypes, want))
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "m4q_plant_ilqr_batch")
    for name in ("plant_ilqr_batch", "plant_ilqr_reference"):
        assert getattr(m4q, name) is getattr(plant_ilqr, name)
    for cls in (m4q.QExperiment, m4q.QSynthesis):
        assert callable(cls.ilqr_batch)


# ---------------------------------------------------------------- the Python wrappers
no_library = sqp_host.no_library


@pytest.mark.parametrize("change", sqp_host.WRAPPER_BAD,
                         ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", "")) for k, v in c.items()))
def test_wrapper_refuses_bad_arguments(no_library, change):
    for fn in (m4q.plant_ilqr_batch, m4q.plant_ilqr_reference):
        with pytest.raises(ValueError):
            fn(**dict(sqp_host._args(), **change))


def test_wrapper_refuses_wrong_types_and_experiments(no_library):
    _args = sqp_host._args
    for change in (dict(U0=np.zeros((3, 4, 2), complex)), dict(U_bm=np.zeros((4, 2), complex)), dict(du=0.1, u_prev=np.zeros(2, complex)),
                   dict(iters=2.5), dict(steps=True)):
        with pytest.raises(TypeError):
            m4q.plant_ilqr_batch(**dict(_args(), **change))
    a = _args()
    rest = (a["x0"], a["U0"], 0.25, a["X_bm"], a["U_bm"], a["Q_ls"], a["R_ls"], 1.0)
    with pytest.raises(ValueError):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).ilqr_batch(*rest)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    exp.set("c_ops", [np.eye(3)])
    with pytest.raises(ValueError):                                # collapse operators: a generator plant
        exp.ilqr_batch(*rest)


class _Fake:
    def __init__(self, seen):
        self.seen = seen

    def m4q_plant_ilqr_batch(self, *a):
        self.seen["ilqr"] = a
        return 0

    def m4q_last_error(self):
        return b""


def test_the_wrapper_stages_what_the_entry_point_takes(monkeypatch):
    seen = {}
    monkeypatch.setattr(_lib, "lib", lambda: _Fake(seen))
    c, args, kw = ic.problem("9-2", "per", 5, 6)
    out = m4q.plant_ilqr_batch(*args, iters=7, exact=True, gains=True, **kw)
    f = seen["ilqr"]
    assert len(f) == 33 and f[:5] == (5, 9, 2, _lib.PLANT_HAMILTONIAN, 6)
    assert f[8] == 1 and f[9] is None and f[12] == 1 and f[13] == (_lib.QP_DU_BAND | _lib.QP_EXACT_BOX) and f[14] == c.sat
    assert f[15] == kw["du"] and f[18] == 1 and f[22:25] == (7, ic.STEPS, ic.TOL_SQP) and all(p is not None for p in f[25:])
    assert sorted(out) == sorted(["X", "U", "cost", "cost_hist", "alpha_hist", "n_iter", "status", "gains"])
    assert out["X"].shape == (5, 7, 9) and out["U"].shape == (5, 6, 2) and out["cost_hist"].shape == (5, 8)
    assert out["alpha_hist"].shape == (5, 7) and out["n_iter"].dtype == out["status"].dtype == np.int32 and out["gains"].shape == (5, 6, 10, 2)
    c, args, kw = ic.problem("9-2", "shared", 5, 6)
    out = m4q.QExperiment(c.op0, list(c.ops)).ilqr_batch(args[0], args[1], args[4], *args[5:], u_scale=kw["u_scale"])
    f = seen["ilqr"]
    assert f[8] == 0 and f[9] is not None and f[12] == 0 and f[13] == 0 and f[15] == 0.0 and f[21] is None and f[22:25] == (10, 6, 1e-9)
    assert out["gains"] is None and f[32] is None

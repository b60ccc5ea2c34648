"""The SQP on the plant itself (m4q_plant_sqp_batch) without a GPU: the NumPy / SciPy definition of mpc4quantum_amd/plant_sqp.py held
to what it must be - a monotone descent of the true cost along a descent direction of the gradient that tests/test_grad_host.py
holds to central differences, with converged points as fixed points - the decision margins and the amplification of every case
tests/test_gpu_plant_sqp.py runs, every refusal of the C entry point (all come back before a device is asked for), and the
prototype against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, plant_linearize, plant_sqp
from tests import grad_cases as gc
from tests import plant_sqp_cases as sc

DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"m4q_plant_sqp_batch"
CASES = sc.all_cases()
IDS = [sc.case_id(*c) for c in CASES]


def _rel(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(want).max())


def _member(args, kw, b):
    """(x0, controls scale, op0, ops, dts, X_bm, U_bm) of member b of a problem."""
    x0, U0, op0, ops, ts, X_bm, U_bm = args[:7]
    T = U0.shape[-2]
    dts = np.full(T, ts) if np.ndim(ts) == 0 else np.diff(ts)
    s = np.ones(U0.shape[-1]) if kw["u_scale"] is None else kw["u_scale"][b]
    per = op0.ndim == 3
    return (x0[b], s, op0[b] if per else op0, ops[b] if per else ops, dts, X_bm[b] if X_bm.ndim == 3 else X_bm,
            U_bm[b] if U_bm.ndim == 3 else U_bm)


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cost_never_increases_and_is_the_cost_of_the_returned_controls(case):
    name, variant, B, T, exact = case
    c, args, kw = sc.problem(name, variant, B, T)
    ref, trace = sc.reference(*case, 3)
    assert np.all(np.diff(ref["cost_hist"], axis=1) <= 0)
    assert np.array_equal(ref["cost_hist"][:, -1], ref["cost"])
    lo, hi = sc.bounds(args, kw)
    assert np.all(ref["U"] >= lo) and np.all(ref["U"] <= hi)
    Q, R = args[7], args[8]
    Ql, Rl = np.broadcast_to(Q, (T + 1,) + Q.shape), np.broadcast_to(R, (T,) + R.shape)
    for b in range(B):
        x0, s, op0, ops, dts, Xb, Ub = _member(args, kw, b)
        X = gc.plant_chain(c, x0, s * ref["U"][b], op0, ops, dts)          # the independent step (the oracle's)
        assert _rel(X, ref["X"][b]) <= 1e-12
        J = plant_linearize._objective(X, ref["U"][b], Xb, Ub, Ql, Rl)
        assert abs(J - ref["cost"][b]) <= 1e-12 * max(1.0, abs(J))
    assert ref["cost_hist"][:, -1].sum() < ref["cost_hist"][:, 0].sum()


@pytest.mark.parametrize("name", ["4-1", "9-2", "16-1-process"])
def test_the_step_is_a_descent_direction_of_the_true_cost(name):
    """exact=True and a terminal-only cost: the true gradient is plant_rollout_grad_reference's (figure "last", W = Q_T) plus
    2 R (U - U_bm), and the first QP's step goes down it for every member."""
    B, T = 5, 6
    c, args, kw = sc.problem(name, "shared", B, T)
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    Ql = np.zeros((T + 1,) + Q.shape, dtype=complex)
    Ql[T] = Q
    trace = []
    m4q.plant_sqp_reference(x0, U0, op0, ops, ts, X_bm, U_bm, Ql, R, sat, iters=1, exact=True, trace=trace, **kw)
    lo, hi = sc.bounds(args, kw)
    U = np.minimum(np.maximum(np.broadcast_to(U0, (B, T, c.m)), lo), hi)
    g = m4q.plant_rollout_grad_reference(x0, U, op0, ops, ts, Q, X_bm[T][None], c.kind, u_scale=kw["u_scale"], figure="last")["grad"]
    g = g + 2 * np.einsum('kl,btl->btk', R.real, U - U_bm)
    assert [rec["i"] for rec in trace] == [0] * B
    for rec in trace:
        slope = float(np.sum(g[rec["b"]] * (rec["U_qp"] - U[rec["b"]])))
        print("%s member %d: g . (U_qp - U) = %.3e (|g| = %.3e, |D| = %.3e)"
              % (name, rec["b"], slope, np.abs(g[rec["b"]]).max(), np.abs(rec["U_qp"] - U[rec["b"]]).max()))
        assert slope < 0


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
def test_a_converged_point_is_a_fixed_point(exact):
    c, args, kw = sc.problem("9-2", "per", 5, 6)
    kw = dict(kw, tol=1e-6)
    first = m4q.plant_sqp_reference(*args, iters=64, exact=exact, **kw)
    assert np.all(first["status"] == plant_sqp.STATUS_CONVERGED), (first["status"], first["n_iter"])
    again = m4q.plant_sqp_reference(args[0], first["U"], *args[2:], iters=64, exact=exact, **kw)
    assert np.all((again["status"] == plant_sqp.STATUS_CONVERGED) | (again["status"] == plant_sqp.STATUS_NO_DESCENT))
    assert np.all(again["n_iter"] <= 1)
    assert np.all(again["cost"] <= first["cost"])
    assert np.all(first["cost"] - again["cost"] <= kw["tol"] * first["cost"])
    print("restart (%s): status %s, n_iter %s, relative decrease %s" % ("exact" if exact else "clipped", again["status"], again["n_iter"],
                                                                        (first["cost"] - again["cost"]) / first["cost"]))


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
def test_gains_are_the_qp_s_at_the_returned_point(exact):
    c, args, kw = sc.problem("9-2", "per", 5, 6)
    ref, _ = sc.reference("9-2", "per", 5, 6, exact, 3)
    x0, U0, op0, ops, ts, X_bm, U_bm, Q, R, sat = args
    want = m4q.plant_quad_program_reference(ref["X"][:, :6], ref["U"], op0, ops, ts, X_bm, U_bm, Q, R, sat, du=kw["du"], u_prev=kw["u_prev"],
                                            x_init=x0, kind=c.kind, exact=exact)[3]
    assert np.array_equal(ref["gains"], want)
    less = m4q.plant_sqp_reference(*args, iters=3, exact=exact, **kw)
    assert less["gains"] is None and all(np.array_equal(less[k], ref[k]) for k in less if k != "gains")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decision_margins_of_the_gpu_cases(case):
    """No decision of the definition in a GPU case is a rounding decision: every member is compared on the device."""
    ref, trace = sc.reference(*case, 3)
    gap, descent, stop = sc.margins(trace, sc.TOL_SQP)
    print("%s: best against the next candidate %.2e, J_j* < J by %.2e, dec against tol J %.2e (relative to J); alphas %s"
          % (sc.case_id(*case), gap, descent, stop, sorted(set(ref["alpha_hist"].reshape(-1)))))
    assert min(gap, descent, stop) >= sc.MARGIN
    assert np.all((ref["status"] == plant_sqp.STATUS_ITERS) == (ref["n_iter"] == 3))
    assert np.all((ref["status"] == plant_sqp.STATUS_ITERS) | (ref["status"] == plant_sqp.STATUS_NO_DESCENT))
    one, trace1 = sc.reference(*case[:5], 1)
    assert min(sc.margins(trace1, sc.TOL_SQP)) >= sc.MARGIN
    assert np.array_equal(one["U"], np.stack([rec["Us"][int(np.argmin(rec["Js"]))] for rec in trace if rec["i"] == 0]))


def test_the_converged_start_stops_with_a_clear_margin():
    """From a converged U the decrease an accepted step can make is rounding (~1e-16 of J) against tol = 1e-9: status 1 or 2."""
    c, args, kw, exact = sc.converged_start()
    trace = []
    out = m4q.plant_sqp_reference(*args, iters=3, exact=exact, trace=trace, **kw)
    assert np.all((out["status"] == plant_sqp.STATUS_CONVERGED) | (out["status"] == plant_sqp.STATUS_NO_DESCENT))
    assert np.all(out["n_iter"] <= 1)
    for rec in trace:
        dec = (rec["J"] - min(rec["Js"])) / rec["J"]
        print("member %d: relative decrease %.2e against tol %.0e" % (rec["b"], dec, kw["tol"]))
        assert dec <= 1e-3 * kw["tol"]
    same = out["status"] == plant_sqp.STATUS_NO_DESCENT
    assert np.array_equal(out["U"][same], args[1][same])


def _perturbed(rng, a):
    return a * (1 + sc.EPS * rng.uniform(-1, 1, a.shape))


def amplification(case):
    name, variant, B, T, exact = case
    c, args, kw = sc.problem(name, variant, B, T)
    ref, _ = sc.reference(*case, 3)
    rng = np.random.default_rng(7400 + CASES.index(case))
    x0, U0, op0, ops = (_perturbed(rng, a) for a in args[:4])
    out = m4q.plant_sqp_reference(x0, U0, op0, ops, *args[4:], iters=3, exact=exact, gains=True, **kw)
    assert np.array_equal(out["alpha_hist"], ref["alpha_hist"]) and np.array_equal(out["status"], ref["status"])
    return max(_rel(out[k], ref[k]) for k in ("X", "U", "cost", "cost_hist", "gains")) / sc.EPS


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_amplification_of_the_gpu_cases(case):
    """The record of tests/plant_sqp_cases.py: AMPLIFICATION is what this test computes (same seeds)."""
    s = amplification(case)
    print('    "%s": %.1f,' % (sc.case_id(*case), s))
    assert np.isfinite(s)
    recorded = sc.AMPLIFICATION[sc.case_id(*case)]
    assert s <= 10 * max(1.0, recorded)                            # (the record is of this computation, up to the platform's expm)


# ---------------------------------------------------------------- the C ABI
def _buf(n, kind=np.float64):
    a = np.zeros(max(int(n), 1), dtype=kind)
    return a, a.ctypes.data_as(DP if kind is np.float64 else IP)


class _Call:
    """One valid m4q_plant_sqp_batch call on host buffers of the right sizes; fields are replaced one at a time."""
    ORDER = ("B", "n", "m", "kind", "T", "dts", "x0", "U0", "u_per", "u_scale", "op0", "ops", "per", "flags", "sat", "du", "X_bm", "U_bm",
             "bm_per", "Q_ls", "R_ls", "u_prev", "iters", "steps", "tol", "X", "U", "cost", "cost_hist", "alpha_hist", "n_iter", "status",
             "gains")

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, T=4, k=3, iters=3):
        self.keep = {}
        b = self._b
        self.v = dict(B=B, n=n, m=m, kind=kind, T=T, dts=b("dts", T), x0=b("x0", 2 * B * n), U0=b("U0", T * m), u_per=0, u_scale=None,
                      op0=b("op0", 2 * k * k), ops=b("ops", 2 * m * k * k), per=0, flags=0, sat=1.0, du=0.0,
                      X_bm=b("Xb", 2 * (T + 1) * n), U_bm=b("Ub", T * m), bm_per=0, Q_ls=b("Q", 2 * (T + 1) * n * n),
                      R_ls=b("R", 2 * T * m * m), u_prev=None, iters=iters, steps=4, tol=1e-9, X=b("X", 2 * B * (T + 1) * n),
                      U=b("U", B * T * m), cost=b("c", B), cost_hist=b("ch", B * (iters + 1)), alpha_hist=b("ah", B * iters),
                      n_iter=b("ni", B, np.int32), status=b("st", B, np.int32), gains=None)

    def _b(self, name, count, kind=np.float64):
        self.keep[name], p = _buf(count, kind)
        return p

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_sqp_batch(*[v[k] for k in self.ORDER])


BAD = [(dict(B=0), b"B and T"), (dict(T=0), b"B and T"), (dict(B=70000, T=70000), b"do not fit"), (dict(dts=None), b"required"),
       (dict(x0=None), b"x0"), (dict(U0=None), b"U0"), (dict(op0=None), b"required"), (dict(ops=None), b"required"),
       (dict(X_bm=None), b"required"), (dict(U_bm=None), b"required"), (dict(Q_ls=None), b"required"), (dict(R_ls=None), b"required"),
       (dict(X=None), b"required"), (dict(U=None), b"required"), (dict(cost=None), b"required"), (dict(cost_hist=None), b"required"),
       (dict(alpha_hist=None), b"required"), (dict(n_iter=None), b"required"), (dict(status=None), b"required"),
       (dict(sat=0.0), b"sat"), (dict(sat=float("nan")), b"sat"), (dict(flags=8), b"qp_flags"), (dict(flags=-1), b"qp_flags"),
       (dict(flags=_lib.QP_EXACT_BOX | _lib.QP_REF_LQR), b"M4Q_QP_REF_LQR"), (dict(kind=0), b"plant_kind"), (dict(kind=4), b"plant_kind"),
       (dict(kind=_lib.PLANT_PROCESS), b"fourth power"),
       (dict(iters=0), b"iters"), (dict(iters=65), b"iters"), (dict(iters=-1), b"iters"), (dict(steps=0), b"steps"), (dict(steps=9), b"steps"),
       (dict(tol=-1e-9), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(tol=float("inf")), b"tol")]


@pytest.mark.parametrize("change,word", BAD, ids=[str(c) for c, _ in BAD])
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
        return                                                    # (with a device these calls run: tests/test_gpu_plant_sqp.py)
    for call in (_Call(), _Call(n=4, m=1, k=2), _Call(n=16, m=3, k=4), _Call(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2), _Call(iters=64)):
        B, m = call.v["B"], call.v["m"]
        assert call() == _lib.E_NODEVICE
        assert call(flags=_lib.QP_EXACT_BOX) == _lib.E_NODEVICE
        assert call(flags=_lib.QP_DU_BAND, du=0.5, u_prev=call._b("up", B * m)) == _lib.E_NODEVICE
        assert call(u_scale=call._b("sc", B * m), gains=call._b("g", 1), tol=0.0, steps=1) == _lib.E_NODEVICE
        assert call(steps=8) == _lib.E_NODEVICE


def test_prototype_agrees_with_the_header():
    header = open(os.path.join(ROOT, "include", "m4q.h")).read()
    decl = re.search(r"M4Q_API int m4q_plant_sqp_batch\((.*?)\);", header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    kinds = {"int32_t": _lib._i32, "double": ctypes.c_double, "const double*": _lib._dp, "double*": _lib._dp, "int32_t*": _lib._ip}
    want = [kinds[p.rsplit(" ", 1)[0]] for p in params]
    restype, argtypes = _lib.PROTOTYPES["m4q_plant_sqp_batch"]
    assert restype is ctypes.c_int and len(argtypes) == len(want) == 33
    assert all(a is w for a, w in zip(argtypes, want))
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "B", "dim_x", "dim_u", "plant_kind", "T", "dts", "x0", "U0", "u_per_instance", "u_scale", "op0", "ops", "plant_per_instance",
        "qp_flags", "sat", "du", "X_bm", "U_bm", "bm_per_instance", "Q_ls", "R_ls", "u_prev", "iters", "steps", "tol", "X", "U", "cost",
        "cost_hist", "alpha_hist", "n_iter", "status", "gains"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "m4q_plant_sqp_batch")
    for name in ("plant_sqp_batch", "plant_sqp_reference"):
        assert getattr(m4q, name) is getattr(plant_sqp, name)
    for cls in (m4q.QExperiment, m4q.QSynthesis):
        assert callable(cls.sqp_batch)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: arguments are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, T=4, n=9, m=2, k=3):
    return dict(x0=np.zeros((B, n), complex), U0=np.zeros((B, T, m)), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex),
                dt_or_ts=0.25, X_bm=np.zeros((T + 1, n), complex), U_bm=np.zeros((T, m)), Q_ls=np.eye(n), R_ls=np.eye(m), sat=1.0)


WRAPPER_BAD = [dict(x0=np.zeros(9)), dict(x0=np.zeros((3, 4, 9))), dict(U0=np.zeros(4)), dict(U0=np.zeros((2, 4, 2))), dict(op0=np.zeros((2, 2))),
               dict(dt_or_ts=np.zeros(4)), dict(X_bm=np.zeros((4, 9))), dict(U_bm=np.zeros((4, 1))), dict(Q_ls=np.eye(4)),
               dict(R_ls=np.zeros((5, 2, 2))), dict(sat=0.0), dict(sat=None), dict(du=0.1, u_prev=np.zeros((2, 2))),
               dict(du=0.0, u_prev=np.zeros(2)), dict(u_scale=np.ones((3, 1))), dict(kind=_lib.PLANT_GENERATOR),
               dict(kind=_lib.PLANT_PROCESS), dict(kind=7), dict(iters=0), dict(iters=65), dict(steps=0), dict(steps=9), dict(tol=-1.0),
               dict(tol=float("nan")), dict(tol=float("inf"))]


@pytest.mark.parametrize("change", WRAPPER_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", "")) for k, v in c.items()))
def test_wrapper_refuses_bad_arguments(no_library, change):
    for fn in (m4q.plant_sqp_batch, m4q.plant_sqp_reference):
        with pytest.raises(ValueError):
            fn(**dict(_args(), **change))


def test_wrapper_refuses_wrong_types_and_experiments(no_library):
    for change in (dict(U0=np.zeros((3, 4, 2), complex)), dict(U_bm=np.zeros((4, 2), complex)), dict(du=0.1, u_prev=np.zeros(2, complex)),
                   dict(iters=2.5), dict(steps=True)):
        with pytest.raises(TypeError):
            m4q.plant_sqp_batch(**dict(_args(), **change))
    a = _args()
    rest = (a["x0"], a["U0"], 0.25, a["X_bm"], a["U_bm"], a["Q_ls"], a["R_ls"], 1.0)
    with pytest.raises(ValueError):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).sqp_batch(*rest)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    exp.set("c_ops", [np.eye(3)])
    with pytest.raises(ValueError):                                # collapse operators: a generator plant
        exp.sqp_batch(*rest)


class _Fake:
    def __init__(self, seen):
        self.seen = seen

    def m4q_plant_sqp_batch(self, *a):
        self.seen["sqp"] = a
        return 0

    def m4q_last_error(self):
        return b""


def test_the_wrapper_stages_what_the_entry_point_takes(monkeypatch):
    seen = {}
    monkeypatch.setattr(_lib, "lib", lambda: _Fake(seen))
    c, args, kw = sc.problem("9-2", "per", 5, 6)
    out = m4q.plant_sqp_batch(*args, iters=7, exact=True, gains=True, **kw)
    f = seen["sqp"]
    assert len(f) == 33 and f[:5] == (5, 9, 2, _lib.PLANT_HAMILTONIAN, 6)
    assert f[8] == 1 and f[9] is None and f[12] == 1 and f[13] == (_lib.QP_DU_BAND | _lib.QP_EXACT_BOX) and f[14] == c.sat
    assert f[15] == kw["du"] and f[18] == 1 and f[22:25] == (7, sc.STEPS, sc.TOL_SQP) and all(p is not None for p in f[25:])
    assert out["X"].shape == (5, 7, 9) and out["U"].shape == (5, 6, 2) and out["cost_hist"].shape == (5, 8)
    assert out["alpha_hist"].shape == (5, 7) and out["n_iter"].dtype == out["status"].dtype == np.int32 and out["gains"].shape == (5, 6, 10, 2)
    c, args, kw = sc.problem("9-2", "shared", 5, 6)
    out = m4q.QExperiment(c.op0, list(c.ops)).sqp_batch(args[0], args[1], args[4], *args[5:], u_scale=kw["u_scale"])
    f = seen["sqp"]
    assert f[8] == 0 and f[9] is not None and f[12] == 0 and f[13] == 0 and f[15] == 0.0 and f[21] is None and f[22:25] == (10, 6, 1e-9)
    assert out["gains"] is None and f[32] is None

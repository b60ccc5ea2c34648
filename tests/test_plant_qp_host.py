"""The QP on the plant's own linearisation (m4q_plant_quad_program_batch) without a GPU: the NumPy definition of
mpc4quantum_amd/plant_linearize.py against the oracle's three independent solvers on the definition's Jacobians, every refusal of the
C entry point (all come back before a device is asked for), the prototype against the header, and what
FeedbackLaw.along_plant_trajectory_fused hands to the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, plant_linearize
from oracle import m4q_oracle as orc
from tests import grad_cases as gc

DP = ctypes.POINTER(ctypes.c_double)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
WHO = b"m4q_plant_quad_program_batch"


# ---------------------------------------------------------------- the definition
_CASES = {}


def _case(name):
    """B = 3, T = 6, per-member operators, u_scale != 1, a non-uniform grid; the Jacobians of the definition; the unbounded solve."""
    if name not in _CASES:
        c = gc.plant_case(name)
        rng = np.random.default_rng(9900 + gc.PLANT_NAMES.index(name))
        B, T = 3, 6
        # (density matrices and process vectors, as are the targets: on such problems the real part of the complex policy is the
        #  optimal real control, which is what makes the sweep comparable with solvers over real controls)
        X = c.states(rng, B * T).reshape(B, T, c.n)
        U =0.5 * c.sat * rng.uniform(-1, 1, (B, T, c.m))
        op0, ops = c.member_ops(rng, B)
        sc = 1 + 0.1 * rng.standard_normal((B, c.m))
        ts = gc.grid(rng, T, c.dt)
        X_bm = c.states(rng, B * (T + 1)).reshape(B, T + 1, c.n)
        U_bm = 0.1 * c.sat * rng.uniform(-1, 1, (B, T, c.m))
        Q, R = np.identity(c.n), 0.1 * np.identity(c.m)
        lin = m4q.plant_linearize_reference(X, U, op0, ops, ts, c.kind, u_scale=sc)
        plant = (X, U, op0, ops, ts)
        far = 1e3 * c.sat
        free = m4q.plant_quad_program_reference(*plant, X_bm, U_bm, Q, R, far, kind=c.kind, u_scale=sc)
        assert np.abs(free[1]).max() < 0.1 * far                   # the bound is far from every control
        _CASES[name] = (c, plant, sc, X_bm, U_bm, Q, R, lin, far, free)
    return _CASES[name]


def _lists(T, Q, R):
    return [Q.astype(complex)] * (T + 1), [R.astype(complex)] * T


def _rel(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", gc.PLANT_NAMES)
def test_unbounded_definition_against_the_dense_kkt_solve(name):
    c, plant, sc, X_bm, U_bm, Q, R, (A, Bm, D), far, (Xo, Uo, cost, gains) = _case(name)
    B, T = U_bm.shape[:2]
    Ql, Rl = _lists(T, Q, R)
    for b in range(B):
        Xk, Uk = orc.kkt_quad_program(plant[0][b, 0], X_bm[b].T, U_bm[b].T, Ql, Rl, list(A[b]), list(Bm[b]), list(D[b]))
        ex, eu = _rel(Xo[b].T, Xk), _rel(Uo[b].T, Uk)
        print("%s member %d: against the KKT solve max|dX| %.2e, max|dU| %.2e (max|U| = %.3e)" % (name, b, ex, eu, np.abs(Uk).max()))
        assert ex <= TOL and eu <= TOL


@pytest.mark.parametrize("band", [False, True], ids=["box", "band"])
@pytest.mark.parametrize("name", gc.PLANT_NAMES)
def test_bounded_definition_against_the_oracle_s_clipped_and_exact_solvers(name, band):
    """sat at half the largest control of the unbounded solve: bounds are active in both modes."""
    c, plant, sc, X_bm, U_bm, Q, R, (A, Bm, D), far, free = _case(name)
    B, T, m = U_bm.shape
    n = c.n
    Ql, Rl = _lists(T, Q, R)
    sat = 0.5 * np.abs(free[1]).max()
    du = 0.3 * sat if band else None
    u_prev = 0.2 * sat * np.ones((B, m)) if band else None
    x_init = plant[0][:, 0] + 0.01
    kw = dict(du=du, u_prev=u_prev, x_init=x_init, kind=c.kind, u_scale=sc)
    Xc, Uc, cc, gc_ = m4q.plant_quad_program_reference(*plant, X_bm, U_bm, Q, R, sat, **kw)
    Xe, Ue, ce, ge = m4q.plant_quad_program_reference(*plant, X_bm, U_bm, Q, R, sat, exact=True, **kw)
    assert gc_.shape == ge.shape == (B, T, n + 1, m)
    pinned = 0
    for b in range(B):
        args = (x_init[b], X_bm[b].T, U_bm[b].T, Ql, Rl, list(A[b]), list(Bm[b]), list(D[b]), None if not band else u_prev[b], sat, du)
        Xr, Ur, cr, gr = orc.quad_program(*args)
        assert max(_rel(Xc[b].T, Xr), _rel(Uc[b].T, Ur), _rel(cc[b], cr)) <= TOL
        assert _rel(gc_[b], np.stack([g.T for g in gr])) <= TOL
        Xr, Ur, cr = orc.exact_quad_program(*args)
        assert max(_rel(Xe[b].T, Xr), _rel(Ue[b].T, Ur), _rel(ce[b], cr)) <= TOL
        assert ce[b] <= cc[b] * (1 + 1e-12)
        on = np.abs(np.abs(Ue[b]) - sat) <= 1e-12 * sat
        pinned += int(on.sum())
        # a free control's slot holds its feedback row: the exact solution follows its own policy
        z = np.concatenate([Xe[b, :T] - X_bm[b, :T], np.ones((T, 1))], axis=1)
        u_pol = np.einsum('tck,tc->tk', ge[b], z).real + U_bm[b]
        lo, hi = np.full((T, m), -sat), np.full((T, m), sat)
        if band:
            lo[0], hi[0] = np.maximum(lo[0], u_prev[b] - du), np.minimum(hi[0], u_prev[b] + du)
        at = (Ue[b] <= lo) | (Ue[b] >= hi)
        assert np.abs((u_pol - Ue[b])[~at]).max(initial=0.0) <= 1e-9 * max(1.0, sat)
        # a pinned control's slot holds its multiplier: outward on the side it is pinned on
        mu = np.einsum('tck,tc->tk', ge[b], z).real
        assert np.all(mu[Ue[b] >= hi] <= 0) and np.all(mu[Ue[b] <= lo] >= 0)
    assert pinned > 0
    assert np.abs(Ue).max() <= sat and np.abs(Uc).max() <= sat


def test_gains_false_and_x_init_default():
    c, plant, sc, X_bm, U_bm, Q, R, lin, far, free = _case("4-2")
    out = m4q.plant_quad_program_reference(*plant, X_bm, U_bm, Q, R, far, kind=c.kind, u_scale=sc, gains=False, x_init=plant[0][:, 0])
    assert out[3] is None
    for g, f in zip(out[:3], free[:3]):
        assert np.array_equal(g, f)


# ---------------------------------------------------------------- the C ABI
def _buf(n):
    a = np.zeros(max(int(n), 1), dtype=np.float64)
    return a, a.ctypes.data_as(DP)


class _Call:
    """One valid m4q_plant_quad_program_batch call on host buffers of the right sizes; fields are replaced one at a time."""
    ORDER = ("B", "n", "m", "kind", "T", "dts", "X", "U", "u_per", "u_scale", "op0", "ops", "per", "flags", "sat", "du", "x_init",
             "X_bm", "U_bm", "bm_per", "Q_ls", "R_ls", "u_prev", "X_opt", "U_opt", "cost", "gains")

    def __init__(self, B=3, n=9, m=2, kind=_lib.PLANT_HAMILTONIAN, T=4, k=3):
        self.keep = {}
        b = self._b
        self.v = dict(B=B, n=n, m=m, kind=kind, T=T, dts=b("dts", T), X=b("X", 2 * B * T * n), U=b("U", T * m), u_per=0, u_scale=None,
                      op0=b("op0", 2 * k * k), ops=b("ops", 2 * m * k * k), per=0, flags=0, sat=1.0, du=0.0, x_init=None,
                      X_bm=b("Xb", 2 * (T + 1) * n), U_bm=b("Ub", T * m), bm_per=0, Q_ls=b("Q", 2 * (T + 1) * n * n),
                      R_ls=b("R", 2 * T * m * m), u_prev=None, X_opt=b("Xo", 2 * B * (T + 1) * n), U_opt=b("Uo", B * T * m),
                      cost=b("c", B), gains=None)

    def _b(self, name, count):
        self.keep[name], p = _buf(count)
        return p

    def __call__(self, **change):
        v = dict(self.v, **change)
        return _lib.lib().m4q_plant_quad_program_batch(*[v[k] for k in self.ORDER])


BAD = [dict(B=0), dict(B=-2), dict(T=0), dict(T=-1), dict(B=70000, T=70000), dict(dts=None), dict(X=None), dict(U=None), dict(op0=None),
       dict(ops=None), dict(X_bm=None), dict(U_bm=None), dict(Q_ls=None), dict(R_ls=None), dict(X_opt=None), dict(U_opt=None),
       dict(cost=None), dict(sat=0.0), dict(sat=-1.0), dict(sat=float("nan")), dict(flags=8), dict(flags=-1),
       dict(flags=_lib.QP_EXACT_BOX | _lib.QP_REF_LQR), dict(kind=0), dict(kind=4), dict(kind=-1), dict(kind=_lib.PLANT_PROCESS)]


@pytest.mark.parametrize("change", BAD, ids=str)
def test_refuses_bad_arguments(change):
    """(kind = PROCESS on n = 9: not a fourth power.)"""
    assert _Call()(**change) == _lib.E_BADARG
    assert WHO in _lib.lib().m4q_last_error()


def test_refuses_what_has_no_kernel():
    L = _lib.lib()
    for call, word in ((_Call(n=25, k=5), b"no kernel"), (_Call(n=9, m=3), b"no kernel"), (_Call(n=8, m=2, k=2), b"not a square"),
                       (_Call(n=9, kind=_lib.PLANT_GENERATOR, k=9), b"m4q_discretize_batch + m4q_linearize_batch + m4q_quad_program_batch"),
                       (_Call(n=16, m=2, k=4), b"plant-only")):
        assert call() == _lib.E_UNSUPPORTED
        assert WHO in L.m4q_last_error() and word in L.m4q_last_error()
    # the exact mode's workspace limit, before a device is asked for: 2 x 16 n B (T + 1) bytes below 4 GiB
    call = _Call(n=16, m=1, k=4)
    assert call(B=4_000_000, T=3, flags=_lib.QP_EXACT_BOX) == _lib.E_BADARG
    assert WHO in L.m4q_last_error() and b"4 GiB" in L.m4q_last_error()


def test_valid_calls_reach_the_device_check():
    """Every optional input given or NULL, the exact mode, both plants: nothing but the missing device refuses them."""
    if _lib.device_count() > 0:
        return                                                    # (with a device these calls run: tests/test_gpu_plant_qp.py)
    for call in (_Call(), _Call(n=4, m=1, k=2), _Call(n=16, m=3, k=4), _Call(n=16, m=1, kind=_lib.PLANT_PROCESS, k=2)):
        B, n, m = call.v["B"], call.v["n"], call.v["m"]
        assert call() == _lib.E_NODEVICE
        assert call(flags=_lib.QP_EXACT_BOX) == _lib.E_NODEVICE
        assert call(flags=_lib.QP_DU_BAND, du=0.5, u_prev=call._b("up", B * m)) == _lib.E_NODEVICE
        assert call(x_init=call._b("xi", 2 * B * n), u_scale=call._b("sc", B * m), gains=call._b("g", 1)) == _lib.E_NODEVICE
        assert call(T=1) == _lib.E_NODEVICE and call(B=1) == _lib.E_NODEVICE


def test_prototype_agrees_with_the_header():
    header = open(os.path.join(ROOT, "include", "m4q.h")).read()
    decl = re.search(r"M4Q_API int m4q_plant_quad_program_batch\((.*?)\);", header, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    kinds = {"int32_t": _lib._i32, "double": ctypes.c_double, "const double*": _lib._dp, "double*": _lib._dp}
    want = [kinds[p.rsplit(" ", 1)[0]] for p in params]
    restype, argtypes = _lib.PROTOTYPES["m4q_plant_quad_program_batch"]
    assert restype is ctypes.c_int and len(argtypes) == len(want) == 27
    assert all(a is w for a, w in zip(argtypes, want))
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "B", "dim_x", "dim_u", "plant_kind", "T", "dts", "X", "U", "u_per_instance", "u_scale", "op0", "ops", "plant_per_instance",
        "qp_flags", "sat", "du", "x_init", "X_bm", "U_bm", "bm_per_instance", "Q_ls", "R_ls", "u_prev", "X_opt", "U_opt", "cost", "gains"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "m4q_plant_quad_program_batch")
    for name in ("plant_quad_program_batch", "plant_quad_program_reference"):
        assert getattr(m4q, name) is getattr(plant_linearize, name)
    for cls in (m4q.QExperiment, m4q.QSynthesis, m4q.LExperiment):
        assert callable(cls.quad_program_batch)
    import inspect                                                 # the one-call law is a new name beside the two-call one, same arguments
    assert inspect.signature(m4q.FeedbackLaw.along_plant_trajectory_fused) == inspect.signature(m4q.FeedbackLaw.along_plant_trajectory)


# ---------------------------------------------------------------- the Python wrappers
@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library is a failure: shapes are refused before it is loaded."""
    def boom():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", boom)


def _args(B=3, T=4, n=9, m=2, k=3):
    return dict(X=np.zeros((B, T, n), complex), U=np.zeros((B, T, m)), op0=np.zeros((k, k), complex), ops=np.zeros((m, k, k), complex),
                dt_or_ts=0.25, X_bm=np.zeros((T + 1, n), complex), U_bm=np.zeros((T, m)), Q_ls=np.eye(n), R_ls=np.eye(m), sat=1.0)


WRAPPER_BAD = [dict(X=np.zeros((3, 9))), dict(U=np.zeros((3, 5, 2))), dict(op0=np.zeros((2, 2))), dict(dt_or_ts=np.zeros(4)),
               dict(X_bm=np.zeros((4, 9))), dict(X_bm=np.zeros((2, 5, 9))), dict(U_bm=np.zeros((4, 1))), dict(Q_ls=np.eye(4)),
               dict(Q_ls=np.zeros((4, 9, 9))), dict(R_ls=np.zeros((5, 2, 2))), dict(sat=0.0), dict(sat=None), dict(sat=-1.0),
               dict(du=0.1, u_prev=np.zeros((2, 2))), dict(du=0.0, u_prev=np.zeros(2)), dict(x_init=np.zeros(9)),
               dict(x_init=np.zeros((3, 4))), dict(u_scale=np.ones((3, 1))), dict(kind=_lib.PLANT_GENERATOR), dict(kind=_lib.PLANT_PROCESS),
               dict(kind=7)]


@pytest.mark.parametrize("change", WRAPPER_BAD, ids=lambda c: ",".join("%s%s" % (k, getattr(v, "shape", "")) for k, v in c.items()))
def test_wrapper_refuses_bad_arguments(no_library, change):
    for fn in (m4q.plant_quad_program_batch, m4q.plant_quad_program_reference):
        with pytest.raises(ValueError):
            fn(**dict(_args(), **change))


def test_wrapper_refuses_wrong_types_and_experiments(no_library):
    for change in (dict(U=np.zeros((3, 4, 2), complex)), dict(U_bm=np.zeros((4, 2), complex)), dict(du=0.1, u_prev=np.zeros(2, complex))):
        with pytest.raises(TypeError):
            m4q.plant_quad_program_batch(**dict(_args(), **change))
    a = _args()
    rest = (a["X"], a["U"], 0.25, a["X_bm"], a["U_bm"], a["Q_ls"], a["R_ls"], 1.0)
    with pytest.raises(ValueError):
        m4q.LExperiment(np.eye(9), [np.eye(9)] * 2).quad_program_batch(*rest)
    exp = m4q.QExperiment(np.diag([0.0, 1.0, 2.0]), [np.eye(3), np.eye(3)])
    exp.set("c_ops", [np.eye(3)])
    with pytest.raises(ValueError):                                # collapse operators: a generator plant
        exp.quad_program_batch(*rest)


class _Fake:
    def __init__(self, seen):
        self.seen = seen

    def m4q_plant_linearize_batch(self, *a):
        self.seen["lin"] = a
        return 0

    def m4q_quad_program_batch(self, *a):
        self.seen["qp"] = a
        return 0

    def m4q_plant_quad_program_batch(self, *a):
        self.seen["fused"] = a
        return 0

    def m4q_last_error(self):
        return b""


def _arr(p, count):
    return np.ctypeslib.as_array(p, (count,)).copy()


def test_the_fused_law_stages_what_the_two_calls_stage(monkeypatch):
    """along_plant_trajectory_fused, the library stubbed: the plant side of its one call is the linearisation call's, the
    QP side the QP call's, x_init is X_nom[:, 0], and the law wraps the gains buffer."""
    seen = {}
    monkeypatch.setattr(_lib, "lib", lambda: _Fake(seen))
    rng = np.random.default_rng(9950)
    B, N, n, m = 3, 4, 9, 2
    X_nom = rng.standard_normal((B, N + 1, n)) + 1j * rng.standard_normal((B, N + 1, n))
    U_nom = rng.standard_normal((B, N, m))
    X_targ = rng.standard_normal((N + 1, n)) + 0j
    op0 = rng.standard_normal((B, 3, 3)) + 0j
    ops = rng.standard_normal((m, 3, 3)) + 0j
    ts = np.array([0.0, 0.1, 0.35, 0.4, 1.0])
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    u_prev = rng.standard_normal((B, m))
    Q, R = np.identity(n), 0.1 * np.identity(m)
    for exact in (False, True):
        args = (op0, ops, ts, X_nom, U_nom, X_targ, U_nom, Q, R, 0.7, 0.2)
        kw = dict(u_prev=u_prev, u_scale=sc, exact=exact)
        two = m4q.FeedbackLaw.along_plant_trajectory(*args, **kw)
        one = m4q.FeedbackLaw.along_plant_trajectory_fused(*args, **kw)
        lin, qp, f = seen["lin"], seen["qp"], seen["fused"]
        assert len(f) == 27 and f[:5] == (B, n, m, _lib.PLANT_HAMILTONIAN, N) == lin[:5]
        # the plant side: dts, X, U, u_per_instance, u_scale, op0, ops, plant_per_instance
        for i, count in ((5, N), (6, 2 * B * N * n), (7, B * N * m), (9, B * m), (10, 2 * B * 9), (11, 2 * B * m * 9)):
            assert np.array_equal(_arr(f[i], count), _arr(lin[i], count)), i
        assert f[8] == lin[8] == 1 and f[12] == lin[12] == 1
        # the QP side: flags, sat, du, x_init, X_bm, U_bm, bm_per_instance, Q_ls, R_ls, u_prev
        assert f[13] == qp[4] == (_lib.QP_DU_BAND | (_lib.QP_EXACT_BOX if exact else 0)) and f[14] == qp[5] == 0.7 and f[15] == qp[6] == 0.2
        assert np.array_equal(_arr(f[16], 2 * B * n), _arr(qp[7], 2 * B * n))
        assert np.array_equal(_arr(f[16], 2 * B * n), np.ascontiguousarray(X_nom[:, 0]).view(np.float64).reshape(-1))
        assert f[19] == qp[10] == 1
        for i, j, count in ((17, 8, 2 * B * (N + 1) * n), (18, 9, B * N * m), (20, 11, 2 * (N + 1) * n * n), (21, 12, 2 * N * m * m),
                            (22, 16, B * m)):
            assert np.array_equal(_arr(f[i], count), _arr(qp[j], count)), i
        assert all(p is not None for p in f[23:])
        assert one.gains.shape == two.gains.shape == (B, N, n + 1, m) and one.members == B
        assert np.array_equal(one.x_ref, two.x_ref) and np.array_equal(one.u_ref, two.u_ref) and np.array_equal(one.u_prev, two.u_prev)
    # one nominal, a shared target, no band
    seen.clear()
    one = m4q.FeedbackLaw.along_plant_trajectory_fused(op0[0], ops, 0.25, X_nom[0], U_nom[0], X_targ, U_nom[0], Q, R, 0.7)
    f = seen["fused"]
    assert "lin" not in seen and "qp" not in seen
    assert f[0] == 1 and f[8] == 0 and f[9] is None and f[12] == 0 and f[13] == 0 and f[15] == 0.0 and f[19] == 0 and f[22] is None
    assert one.gains.shape == (N, n + 1, m) and one.members is None


def test_the_fused_law_checks_shapes_before_the_library(no_library):
    n, m, N = 9, 2, 4
    good = dict(op0=np.zeros((3, 3)), ops=np.zeros((m, 3, 3)), dt_or_ts=0.25, X_nom=np.zeros((N + 1, n)), U_nom=np.zeros((N, m)),
                X_targ=np.zeros((N + 1, n)), U_targ=np.zeros((N, m)), Q_ls=np.eye(n), R_ls=np.eye(m), sat=1.0)
    for change in (dict(X_nom=np.zeros((N + 2, n))), dict(U_nom=np.zeros((2, N, m))), dict(X_targ=np.zeros((N, n))),
                   dict(U_targ=np.zeros((N, 1))), dict(Q_ls=np.eye(4)), dict(R_ls=np.zeros((N + 1, m, m))), dict(sat=-1.0),
                   dict(du=0.1, u_prev=np.zeros((2, m))), dict(op0=np.zeros((2, 2))), dict(dt_or_ts=np.zeros(3)),
                   dict(u_scale=np.ones((2, m))), dict(kind=_lib.PLANT_GENERATOR)):
        with pytest.raises(ValueError):
            m4q.FeedbackLaw.along_plant_trajectory_fused(**dict(good, **change))
    with pytest.raises(TypeError):
        m4q.FeedbackLaw.along_plant_trajectory_fused(**dict(good, U_nom=np.zeros((N, m), complex)))

"""The QP on the plant's own linearisation in one device call (plant_factor_kernel + plant_qp_kernel) against the NumPy / SciPy
definition of mpc4quantum_amd/plant_linearize.py, which tests/test_plant_qp_host.py holds to the oracle's three solvers; against the
two-call path it replaces; placement; the second trip of both grids; the feedback law built from it.  Tolerance of DESIGN section 3:
1e-10 max(1, max|ref|).  Every compiled cell: (square shape with a QP kernel) x {Hamiltonian, process where quartic}; shapes as
tests/test_gpu_plant_linearize.py: B in {1, 5} (a ragged quad) and T in {1, 6}."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests.test_plant_qp_host import WHO, _Call

pytestmark = pytest.mark.gpu

TOL = 1e-10
U_TOL = 1e-10                                                       # the project's control tolerance
RUNS = [("shared", 5, 6), ("per", 5, 6), ("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]
NAMES = ("X_opt", "U_opt", "cost", "gains")


def _cells():
    """Every (shape, plant) the library holds the two kernels for, by the names of tests/grad_cases.py."""
    out = []
    for nx, nu in sorted({(nx, nu) for nx, nu, order, plant_only in kv.shapes() if kv.square(nx) and not plant_only}):
        out.append("%d-%d" % (nx, nu))
        if kv.quartic(nx):
            out.append("%d-%d-process" % (nx, nu))
    return out


CELLS = _cells()


def test_the_cells_are_the_built_ones():
    assert CELLS == ["4-1", "4-2", "9-2", "16-1", "16-1-process", "16-3", "16-3-process"]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def _rel(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


_PROBLEMS = {}


def _problem(name, variant, B, T):
    """One run's inputs, its bound and the definition's two answers, computed once and left unchanged.
      shared  one operator set, one control sequence, u_scale, a non-uniform grid, one target
      per     per-member operators, control sequences and targets, a scalar dt, the du band around per-member u_prev
    Nominals are the plant's own trajectories under random controls at half its bound; targets are off them; Q = I, R = 0.1 I;
    sat is half the largest control of the unbounded solve (the definition's, on the CPU), so that bounds are active."""
    key = (name, variant, B, T)
    if key not in _PROBLEMS:
        c = gc.plant_case(name)
        rng = np.random.default_rng(9900 + 13 * CELLS.index(name) + 101 * B + T + (50 if variant == "per" else 0))
        x0 = c.states(rng, B)
        U = 0.5 * c.sat * rng.uniform(-1, 1, (B, T, c.m))
        if variant == "per":
            op0, ops = c.member_ops(rng, B)
            ts, sc = c.dt, None
        else:
            op0, ops = c.op0, c.ops
            U, ts, sc = U[0], gc.grid(rng, T, c.dt), 1 + 0.1 * rng.standard_normal((B, c.m))
        xs = m4q.plant_rollout_batch(x0, U, op0, ops, ts, c.kind, u_scale=sc)["xs"]
        X = np.ascontiguousarray(xs[:, :T])
        shift = 0.03 * rng.uniform(0.5, 1.5, (T + 1, 1))
        X_bm = xs + shift if variant == "per" else xs[0] + shift
        U_bm = np.zeros((B, T, c.m)) if variant == "per" else np.zeros((T, c.m))
        Q, R = np.identity(c.n), 0.1 * np.identity(c.m)
        plant = (X, U, op0, ops, ts)
        kw = dict(kind=c.kind, u_scale=sc)
        free = m4q.plant_quad_program_reference(*plant, X_bm, U_bm, Q, R, 1e3 * c.sat, **kw)
        sat = 0.5 * np.abs(free[1]).max()
        if variant == "per":
            kw.update(du=0.5 * sat, u_prev=0.3 * sat * rng.uniform(-1, 1, (B, c.m)))
        qp = (X_bm, U_bm, Q, R, sat)
        refs = {exact: m4q.plant_quad_program_reference(*plant, *qp, exact=exact, **kw) for exact in (False, True)}
        for a in (X, X_bm, U_bm, Q, R) + refs[False] + refs[True]:
            a.setflags(write=False)
        _PROBLEMS[key] = (c, plant, qp, kw, refs)
    return _PROBLEMS[key]


def _bounds(qp, kw, B, T, m):
    sat = qp[4]
    lo, hi = np.full((B, T, m), -sat), np.full((B, T, m), sat)
    if "du" in kw:
        lo[:, 0], hi[:, 0] = np.maximum(lo[:, 0], kw["u_prev"] - kw["du"]), np.minimum(hi[:, 0], kw["u_prev"] + kw["du"])
    return lo, hi


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("variant,B,T", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", CELLS)
def test_against_the_definition(name, variant, B, T, exact):
    c, plant, qp, kw, refs = _problem(name, variant, B, T)
    ref = refs[exact]
    lo, hi = _bounds(qp, kw, B, T, c.m)
    at = (ref[1] <= lo) | (ref[1] >= hi)
    assert at.any()                                                # a control is pinned in this case
    if exact:
        # the active set is not a rounding decision: no free control of the reference solve within 1e-6 sat of a bound
        gap = np.minimum(ref[1] - lo, hi - ref[1])[~at]
        assert gap.min(initial=np.inf) > 1e-6 * qp[4]
    out = m4q.plant_quad_program_batch(*plant, *qp, exact=exact, **kw)
    errs = []
    for what, got, want in zip(NAMES, out, ref):
        assert got.shape == want.shape and got.dtype == want.dtype and np.isfinite(got).all()
        errs.append(_rel(got, want))
    print("%s %s B=%d T=%d %s: X_opt %.2e, U_opt %.2e, cost %.2e, gains %.2e, each over max(1, max|ref|); %d of %d controls on a bound, "
          "max|gains| = %.3e" % (name, variant, B, T, "exact" if exact else "clipped", *errs, at.sum(), at.size, np.abs(ref[3]).max()))
    assert max(errs) <= TOL
    assert np.all(out[1] >= lo) and np.all(out[1] <= hi)


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("variant,B,T", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", CELLS)
def test_against_the_two_call_path(name, variant, B, T, exact, record_property):
    c, plant, qp, kw, refs = _problem(name, variant, B, T)
    X_bm, U_bm, Q, R, sat = qp
    one = m4q.plant_quad_program_batch(*plant, *qp, exact=exact, **kw)
    A, Bm, D = m4q.plant_linearize_batch(*plant, c.kind, u_scale=kw["u_scale"])
    two = m4q.quad_program_batch(plant[0][:, 0], X_bm.reshape(-1, T + 1, c.n), U_bm.reshape(-1, T, c.m), np.broadcast_to(Q, (T + 1,) + Q.shape),
                                 np.broadcast_to(R, (T,) + R.shape), A, Bm, D, kw.get("u_prev"), sat, kw.get("du"), exact=exact)
    errs = [_rel(g, w) for g, w in zip(one, two)]
    same = all(_bits(g, w) for g, w in zip(one, two))
    record_property("bit_identical_to_the_two_call_path", same)
    print("%s %s B=%d T=%d %s: against the two calls X_opt %.2e, U_opt %.2e, cost %.2e, gains %.2e; bit-identical: %s"
          % (name, variant, B, T, "exact" if exact else "clipped", *errs, same))
    assert max(errs) <= TOL


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("name", CELLS)
def test_a_member_does_not_depend_on_its_place_nor_on_what_is_asked_for(name, exact):
    """Member b alone gives the bits it gives inside B = 5; gains=False gives the same X_opt, U_opt and cost; x_init=None gives the
    bits of x_init = X[:, 0]."""
    c, (X, U, op0, ops, ts), qp, kw, refs = _problem(name, "per", 5, 6)
    full = m4q.plant_quad_program_batch(X, U, op0, ops, ts, *qp, exact=exact, **kw)
    for b in range(5):
        alone = m4q.plant_quad_program_batch(X[b:b + 1], U[b:b + 1], op0[b], ops[b], ts, qp[0][b], qp[1][b], *qp[2:], exact=exact,
                                             du=kw["du"], u_prev=kw["u_prev"][b], kind=c.kind)
        for g, f in zip(alone, full):
            assert _bits(g[0], f[b])
    less = m4q.plant_quad_program_batch(X, U, op0, ops, ts, *qp, exact=exact, gains=False, **kw)
    assert less[3] is None and all(_bits(g, f) for g, f in zip(less[:3], full[:3]))
    given = m4q.plant_quad_program_batch(X, U, op0, ops, ts, *qp, exact=exact, x_init=X[:, 0], **kw)
    assert all(_bits(g, f) for g, f in zip(given, full))
    moved = m4q.plant_quad_program_batch(X, U, op0, ops, ts, *qp, exact=exact, x_init=X[:, 0] + 0.01, **kw)
    assert np.abs(moved[0] - full[0]).max() > 1e-3                  # (x_init is read when it is given)


@pytest.mark.parametrize("name", ["4-1", "16-1-process"])
def test_the_second_trip_of_both_grids(name):
    """Five distinct members tiled to just past QUAD_WRAP members, T = 2: the sweep's quads and the factor kernel's units are past
    their grids' wrap.  The first and last members and the members beside the wrap equal their B = 5 bits, clipped and exact."""
    c, (X, U, op0, ops, ts), qp, kw, refs = _problem(name, "per", 5, 6)
    T = 2
    small = (X[:, :T], U[:, :T], op0, ops, ts, qp[0][:, :T + 1], qp[1][:, :T], *qp[2:])
    B = kv.QUAD_WRAP + 6
    assert B % kv.ROWS and B * T > B > kv.QUAD_WRAP
    tile = lambda a: np.ascontiguousarray(np.resize(a, (B,) + a.shape[1:])) if isinstance(a, np.ndarray) and a.shape[:1] == (5,) else a
    assert _bits(tile(X[:, :T])[5:10], X[:, :T])
    big = tuple(tile(a) for a in small)
    for exact in (False, True):
        want = m4q.plant_quad_program_batch(*small, exact=exact, du=kw["du"], u_prev=kw["u_prev"], kind=c.kind)
        got = m4q.plant_quad_program_batch(*big, exact=exact, du=kw["du"], u_prev=tile(kw["u_prev"]), kind=c.kind)
        for b in (0, 1, kv.QUAD_WRAP - 1, kv.QUAD_WRAP, kv.QUAD_WRAP + 1, B - 2, B - 1):
            for what, g, w in zip(NAMES, got, want):
                assert _bits(g[b], w[b % 5]), (what, b, exact)


@pytest.mark.parametrize("name", ["4-1", "9-2", "16-3"])
def test_the_fused_law_is_the_law_of_the_two_calls(name):
    """The cases of test_the_law_of_the_plant_keeps_its_own_trajectory (tests/test_gpu_plant_linearize.py) through along_plant_trajectory_fused."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(9860 + gc.PLANT_NAMES.index(name))
    N, n, m = 8, c.n, c.m
    Q, R = np.identity(n), 0.1 * np.identity(m)
    x0 = c.states(rng, 1)
    U_nom = 0.5 * c.sat * rng.uniform(-1, 1, (N, m))
    X_nom = m4q.plant_rollout_batch(x0, U_nom, c.op0, c.ops, c.dt, c.kind)["xs"][0]
    args = (c.op0, c.ops, c.dt, X_nom, U_nom, X_nom, U_nom, Q, R, c.sat)
    law = m4q.FeedbackLaw.along_plant_trajectory_fused(*args, kind=c.kind)
    two = m4q.FeedbackLaw.along_plant_trajectory(*args, kind=c.kind)
    assert law.gains.shape == (N, n + 1, m) and law.members is None
    diff = np.abs(law.gains - two.gains).max()
    affine = np.abs(law.gains[:, n, :]).max()
    run = m4q.plant_feedback_batch(x0, law, c.op0, c.ops, c.dt, c.kind)
    du = np.abs(run["us"][0] - U_nom).max()
    print("%s: fused against two calls max|dgains| %.2e (max|K| = %.3e), affine column %.2e, max|us - U_nom| %.2e"
          % (name, diff, np.abs(two.gains[:, :n]).max(), affine, du))
    assert diff <= 1e-10
    assert affine <= U_TOL
    assert du <= U_TOL and np.array_equal(run["clipped"], [0]) and np.array_equal(run["status"], [0])
    assert np.abs(law.gains[:, :n]).max() > 1e-2


def test_the_experiment_wrappers_return_the_module_function_s_arrays():
    c, (X, U, op0, ops, ts), qp, kw, refs = _problem("9-2", "shared", 5, 6)
    want = m4q.plant_quad_program_batch(X, U, c.op0, c.ops, ts, *qp, exact=True, **kw)
    got = m4q.QExperiment(c.op0, list(c.ops)).quad_program_batch(X, U, ts, *qp, u_scale=kw["u_scale"], exact=True)
    assert all(_bits(g, w) for g, w in zip(got, want))
    c, (X, U, op0, ops, ts), qp, kw, refs = _problem("9-2", "per", 5, 6)
    want = m4q.plant_quad_program_batch(X, U, op0, c.ops, ts, *qp, gains=False, **kw)
    got = m4q.QExperiment(c.op0, list(c.ops)).quad_program_batch(X, U, ts, *qp, du=kw["du"], u_prev=kw["u_prev"], gains=False, op0=op0)
    assert got[3] is None and all(_bits(g, w) for g, w in zip(got[:3], want[:3]))
    c, (X, U, op0, ops, ts), qp, kw, refs = _problem("16-1-process", "shared", 5, 6)
    want = m4q.plant_quad_program_batch(X, U, c.op0, c.ops, ts, *qp, **kw)
    got = m4q.QSynthesis(c.op0, list(c.ops)).quad_program_batch(X, U, ts, *qp, u_scale=kw["u_scale"])
    assert all(_bits(g, w) for g, w in zip(got, want))


def test_the_generator_plant_and_the_plant_only_shape_are_refused():
    L = _lib.lib()
    assert _Call(n=9, kind=_lib.PLANT_GENERATOR, k=9)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"m4q_discretize_batch + m4q_linearize_batch + m4q_quad_program_batch" in L.m4q_last_error()
    assert _Call(n=16, m=2, k=4)() == _lib.E_UNSUPPORTED
    assert WHO in L.m4q_last_error() and b"plant-only" in L.m4q_last_error()
    c = gc.plant_case("16-2")
    X, U = np.zeros((2, 3, 16), complex), np.zeros((3, 2))
    with pytest.raises(_lib.M4qError, match="plant-only"):
        m4q.plant_quad_program_batch(X, U, c.op0, c.ops, c.dt, np.zeros((4, 16)), U, np.eye(16), np.eye(2), 1.0)
    with pytest.raises(ValueError, match="generator plant"):
        m4q.plant_quad_program_batch(np.zeros((2, 3, 9), complex), U, np.eye(9), np.stack([np.eye(9)] * 2), 0.1, np.zeros((4, 9)), U,
                                     np.eye(9), np.eye(2), 1.0, kind=_lib.PLANT_GENERATOR)

"""Every plant-side kernel where expm_cols (csrc/m4q_mpc.h) scales and squares: the cases of tests/strong_drive_cases.py - a quiet
member (s = 0) beside members that square up to seven times in one wavefront, s changing along the horizon, the block matrix of
the gradient and linearisation kernels squared, the process and generator plants at s > 0 - against the truth of
tests/golden/strong_drive_truth.npz (mpmath at 40 digits), at the bound each family already has:
    Hamiltonian and process states  rel <= 1e-12        generator states  rel <= 1e-11        (rel: max|d| / max(1, max|ref|))
    gradients, linearisation, QP    1e-10 max(1, max|ref|)                                     
tests/test_strong_drive_host.py holds the preconditions and the fp64 definitions (to a tenth of these bounds); every test here
prints the device's error beside the definition's.  The truth is read, not computed.
The parameter gradient (plant_param_grad_kernel) runs on the same cases with the (1 + p_tot) d block of param_block_expm squared
- in the shared layout with the gains the quiet member's block squares 2 to 5 times while its forward step does not - against
tests/golden/strong_drive_param_truth.npz, at the gradient family's bound."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from oracle import m4q_oracle as orc
from tests import strong_drive_cases as sd

pytestmark = pytest.mark.gpu

TOL = 1e-10
CASES = sd.all_cases()
IDS = [sd.case_id(*c) for c in CASES]
NOT_GEN = [c for c in CASES if not sd.is_generator(c[0])]
NOT_GEN_IDS = [sd.case_id(*c) for c in NOT_GEN]
QP_CASES = sd.all_cases(sd.QP_CELLS)
QP_IDS = [sd.case_id(*c) for c in QP_CASES]


def rel(got, want):
    return np.abs(np.asarray(got) - np.asarray(want)).max() / max(1.0, np.abs(np.asarray(want)).max())


def _bits(a, b):
    """Identical bits (a NaN equals its own bits)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state_bound(cs):
    return 1e-11 if sd.is_generator(cs.cell) else 1e-12


def _s_note(cs):
    s = cs.s()
    return "; ".join("%s s per member (max over t) %s, member 0 along t %s" % (k, a.max(axis=1).tolist(), a[0].tolist()) for k, a in s.items())


_CHAINS = {}


def _definition_chain(cs):
    """The fp64 definition's states (the independent step, interval by interval), computed once per case."""
    if cs.id not in _CHAINS:
        step = orc.plant_step_generator if sd.is_generator(cs.cell) else cs.c.step
        out = np.empty((cs.B, cs.N + 1, cs.n), dtype=complex)
        for b in range(cs.B):
            op0, ops = cs.member_ops(b)
            out[b, 0] = cs.x0[b]
            for t in range(cs.N):
                out[b, t + 1] = step(out[b, t], cs.v[b, t], op0, list(ops), cs.dts[t])
        _CHAINS[cs.id] = out
    return _CHAINS[cs.id]


def _figure_bound(cs, tr, data=None):
    """The bound of a figure q = Re(d^H W d), d = x - f, against the truth: the rollout family's bound of the figure's own
    evaluation, 1e-12 max(1, sum|W| dmax^2) (tests/test_gpu_rollout.py), plus what a state within its bound e = 1e-12 max(1, max|x|)
    (1e-11: generator) can move it, 2 sum|W| dmax e.  data [B|-, N + 1, n]: column t against column t of it, in place of the target."""
    f = data if data is not None else (cs.f[:, None, :] if cs.f.ndim == 2 else cs.f)
    dmax = np.abs(tr["xs"] - f).max()
    w = np.abs(cs.W).sum()
    return 1e-12 * max(1.0, w * dmax ** 2) + 2 * w * dmax * _state_bound(cs) * max(1.0, np.abs(tr["xs"]).max())


# ---------------------------------------------------------------- the step
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_plant_step(key):
    """plant_step_batch from the truth's x_t under the controls the members see, step by step: the mixed quad in one wavefront."""
    cs = sd.case(*key)
    tr = sd.truth(cs)
    ref = _definition_chain(cs)
    worst = 0.0
    for t in range(cs.N):
        out = m4q.plant_step_batch(tr["xs"][:, t], cs.v[:, t], cs.op0, cs.ops, cs.dts[t], cs.kind)
        assert np.isfinite(out).all()
        worst = max(worst, rel(out, tr["xs"][:, t + 1]))
        for b in cs.quiet:                                        # the quiet member alone gives the same bits
            op0, ops = cs.member_ops(b)
            alone = m4q.plant_step_batch(tr["xs"][b:b + 1, t], cs.v[b:b + 1, t], op0[None], ops[None], cs.dts[t], cs.kind)
            assert _bits(alone[0], out[b])
    print("%s: device %.2e, definition (whole chain) %.2e, bound %.1e; %s" % (cs.id, worst, rel(ref, tr["xs"]), _state_bound(cs), _s_note(cs)))
    assert worst <= _state_bound(cs)


# ---------------------------------------------------------------- the rollout and the feedback run
def _rollout(cs, operands=None, **kw):
    x0, us, op0, ops, sc, f = operands or (cs.x0, cs.us, cs.op0, cs.ops, cs.u_scale, cs.f)
    return m4q.plant_rollout_batch(x0, us, op0, ops, cs.ts, cs.kind, u_scale=sc, W=cs.W, target=f, **kw)


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_plant_rollout(key):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    out = _rollout(cs, keep="all", figure="all")
    assert np.isfinite(out["xs"]).all() and _bits(out["xs"][:, 0], cs.x0)
    err, err_q, qb = rel(out["xs"], tr["xs"]), np.abs(out["q"] - tr["q"]).max(), _figure_bound(cs, tr)
    print("%s: xs device %.2e, definition %.2e, bound %.1e; q max|dq| %.2e, bound %.2e; %s"
          % (cs.id, err, rel(_definition_chain(cs), tr["xs"]), _state_bound(cs), err_q, qb, _s_note(cs)))
    assert err <= _state_bound(cs)
    assert err_q <= qb
    none = _rollout(cs, keep="none", figure="all")
    assert set(none) == {"q"} and _bits(none["q"], out["q"])
    for b in cs.quiet:
        alone = _rollout(cs, cs.alone(b), keep="all", figure="all")
        assert _bits(alone["xs"][0], out["xs"][b]) and _bits(alone["q"][0], out["q"][b])


def _law(cs, us):
    """Zero state gains around the strong sequence, no box: the law commands u_ref itself."""
    lead = us.shape[:-2]
    return m4q.FeedbackLaw(np.zeros(lead + (cs.N, cs.n + 1, cs.m), dtype=complex), np.zeros(lead + (cs.N, cs.n), dtype=complex), us, np.inf)


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_plant_feedback(key):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    out = m4q.plant_feedback_batch(cs.x0, _law(cs, cs.us), cs.op0, cs.ops, cs.ts, cs.kind, u_scale=cs.u_scale)
    assert _bits(out["us"], np.broadcast_to(cs.us, (cs.B, cs.N, cs.m)))
    assert np.array_equal(out["status"], np.zeros(cs.B, np.int32)) and np.array_equal(out["clipped"], np.zeros(cs.B, np.int32))
    err = rel(out["xs"], tr["xs"])
    print("%s: xs device %.2e, definition %.2e, bound %.1e; %s" % (cs.id, err, rel(_definition_chain(cs), tr["xs"]), _state_bound(cs), _s_note(cs)))
    assert err <= _state_bound(cs)
    for b in cs.quiet:
        x0, us, op0, ops, sc, _ = cs.alone(b)
        alone = m4q.plant_feedback_batch(x0, _law(cs, us), op0, ops, cs.ts, cs.kind, u_scale=sc)
        assert _bits(alone["xs"][0], out["xs"][b]) and _bits(alone["us"][0], out["us"][b])


# ---------------------------------------------------------------- the gradient
def _grad(cs, figure, operands=None, **kw):
    x0, us, op0, ops, sc, f = operands or (cs.x0, cs.us, cs.op0, cs.ops, cs.u_scale, cs.f)
    return m4q.plant_rollout_grad_batch(x0, us, op0, ops, cs.ts, cs.W, f, cs.kind, u_scale=sc, figure=figure, **kw)


def _objectives(q):
    if q.ndim == 1:
        return 0.0 + q
    J = np.zeros(q.shape[0])
    for t in range(q.shape[1]):
        J = J + q[:, t]
    return J


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("key", NOT_GEN, ids=NOT_GEN_IDS)
def test_plant_gradient(key, figure):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    want = {"q": tr["q"][:, cs.N] if figure == "last" else tr["q"], "grad": tr["grad_" + figure], "grad_scale": tr["gs_" + figure]}
    ref = m4q.plant_rollout_grad_reference(cs.x0, cs.us, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, u_scale=cs.u_scale, figure=figure)
    out = _grad(cs, figure, scale_grad=True)
    for name in ("grad", "grad_scale"):
        err = rel(out[name], want[name])
        print("%s %s %s: device %.2e, definition %.2e, over max(1, max|ref|), max|ref| = %.3e" % (cs.id, figure, name, err,
                                                                                                 rel(ref[name], want[name]), np.abs(want[name]).max()))
        assert out[name].shape == want[name].shape and np.isfinite(out[name]).all()
        assert err <= TOL
    err_q, qb = np.abs(out["q"] - want["q"]).max(), _figure_bound(cs, tr)
    print("%s %s q: max|dq| %.2e, bound %.2e; %s" % (cs.id, figure, err_q, qb, _s_note(cs)))
    assert err_q <= qb
    assert _bits(out["q"], _rollout(cs, keep="none", figure="last" if figure == "last" else "all")["q"])
    if cs.us.ndim == 2 or cs.B == 1:                               # one sequence shared by the ensemble: the reduction
        red = _grad(cs, figure, reduce=True, scale_grad=True)
        assert _bits(red["grad"], m4q.ordered_weighted_sum(out["grad"])) and _bits(red["grad_scale"], out["grad_scale"])
        assert red["q_mean"] == float(m4q.ordered_weighted_sum(_objectives(out["q"]))) and _bits(red["q"], out["q"])
    for b in cs.quiet:
        alone = _grad(cs, figure, cs.alone(b), scale_grad=True)
        assert all(_bits(alone[name][0], out[name][b]) for name in ("q", "grad", "grad_scale"))


# ---------------------------------------------------------------- the linearisation and the QP on it
def _lin_operands(cs, tr, b=None):
    X = np.ascontiguousarray(tr["xs"][:, :cs.N])
    if b is None:
        return X, cs.us, cs.op0, cs.ops, cs.u_scale
    _, us, op0, ops, sc, _ = cs.alone(b)
    return X[b:b + 1], us, op0, ops, sc


@pytest.mark.parametrize("key", NOT_GEN, ids=NOT_GEN_IDS)
def test_plant_linearize(key):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    X, us, op0, ops, sc = _lin_operands(cs, tr)
    want = sd.linearisation(cs, tr, X)
    ref = m4q.plant_linearize_reference(X, us, op0, ops, cs.ts, cs.kind, u_scale=sc)
    out = m4q.plant_linearize_batch(X, us, op0, ops, cs.ts, cs.kind, u_scale=sc)
    errs = []
    for got, w in zip(out, want):
        assert got.shape == w.shape and np.isfinite(got).all()
        errs.append(rel(got, w))
    nxt = np.einsum('btij,btj->bti', out[0], X) + np.einsum('btik,btk->bti', out[1], np.broadcast_to(us, (cs.B, cs.N, cs.m))) + out[2]
    err_x = np.abs(nxt - tr["xs"][:, 1:]).max()
    print("%s: device A %.2e, B %.2e, Delta %.2e; definition A %.2e, B %.2e, Delta %.2e, over max(1, max|ref|), max|B| = %.3e; "
          "A x + B u + Delta against the truth's next state %.2e; %s"
          % (cs.id, *errs, *[rel(g, w) for g, w in zip(ref, want)], np.abs(want[1]).max(), err_x, _s_note(cs)))
    assert max(errs) <= TOL
    assert err_x <= TOL * max(1.0, np.abs(X).max())
    for b in cs.quiet:
        Xb, ub, o0, ok, scb = _lin_operands(cs, tr, b)
        alone = m4q.plant_linearize_batch(Xb, ub, o0, ok, cs.ts, cs.kind, u_scale=scb)
        assert all(_bits(g[0], f[b]) for g, f in zip(alone, out))


def _qp_problem(cs, tr, sat_share):
    """The QP around the truth's trajectory: targets off it (one shared in the shared layout, the members' own in the per
    layout), the strong sequence as control target, Q = I, R = 0.1 I, the box at sat_share of the strong level."""
    rng = np.random.default_rng(7900 + sd.CELLS.index(cs.cell))
    shift = 0.03 * rng.uniform(0.5, 1.5, (cs.N + 1, 1))
    X_bm = tr["xs"] + shift if cs.per else tr["xs"][0] + shift
    return X_bm, cs.us, np.identity(cs.n), 0.1 * np.identity(cs.m), sat_share * cs.sat


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("key", QP_CASES, ids=QP_IDS)
def test_plant_quad_program(key, exact):
    cs = sd.case(*key)
    tr = sd.truth(cs)
    X, us, op0, ops, sc = _lin_operands(cs, tr)
    X_bm, U_bm, Q, R, sat = qp = _qp_problem(cs, tr, 0.6)
    ref = m4q.plant_quad_program_reference(X, us, op0, ops, cs.ts, *qp, kind=cs.kind, u_scale=sc, exact=exact)
    at = np.abs(ref[1]) >= sat
    if exact:                                                      # the active set is not a rounding decision
        assert (sat - np.abs(ref[1]))[~at].min(initial=np.inf) > 1e-6 * sat
    out = m4q.plant_quad_program_batch(X, us, op0, ops, cs.ts, *qp, kind=cs.kind, u_scale=sc, exact=exact)
    A, Bm, D = m4q.plant_linearize_batch(X, us, op0, ops, cs.ts, cs.kind, u_scale=sc)
    T = cs.N
    two = m4q.quad_program_batch(X[:, 0], X_bm.reshape(-1, T + 1, cs.n), U_bm.reshape(-1, T, cs.m), np.broadcast_to(Q, (T + 1,) + Q.shape),
                                 np.broadcast_to(R, (T,) + R.shape), A, Bm, D, None, sat, None, exact=exact)
    errs = [rel(g, w) for g, w in zip(out, ref)]
    errs2 = [rel(g, w) for g, w in zip(out, two)]
    print("%s %s: against the definition X_opt %.2e, U_opt %.2e, cost %.2e, gains %.2e; against the two calls %.2e %.2e %.2e %.2e; "
          "%d of %d controls on a bound; %s" % (cs.id, "exact" if exact else "clipped", *errs, *errs2, at.sum(), at.size, _s_note(cs)))
    assert all(np.isfinite(g).all() for g in out)
    assert max(errs) <= TOL
    assert max(errs2) <= TOL
    assert np.abs(out[1]).max() <= sat
    for b in cs.quiet:
        Xb, ub, o0, ok, scb = _lin_operands(cs, tr, b)
        alone = m4q.plant_quad_program_batch(Xb, ub, o0, ok, cs.ts, X_bm[b] if cs.per else X_bm, ub.reshape(T, cs.m), Q, R, sat, kind=cs.kind,
                                             u_scale=scb, exact=exact)
        assert all(_bits(g[0], f[b]) for g, f in zip(alone, out))


@pytest.mark.parametrize("exact", [False, True], ids=["clipped", "exact"])
@pytest.mark.parametrize("method", ["sqp", "ilqr"])
@pytest.mark.parametrize("key", QP_CASES, ids=QP_IDS)
def test_one_descent_iteration_from_a_strong_start(key, method, exact):
    """One iteration of the SQP / iLQR from the strong sequence, the box at the strong level: the identities that hang on no
    decision.  (Which candidate wins is a rounding decision at this drive and is not compared.)"""
    cs = sd.case(*key)
    tr = sd.truth(cs)
    X_bm, U_bm, Q, R, sat = _qp_problem(cs, tr, 1.0)
    call = m4q.plant_sqp_batch if method == "sqp" else m4q.plant_ilqr_batch
    out = call(cs.x0, cs.us, cs.op0, cs.ops, cs.ts, X_bm, U_bm, Q, R, sat, iters=1, steps=4, kind=cs.kind, u_scale=cs.u_scale, exact=exact)
    for name in ("X", "U", "cost", "cost_hist"):
        assert np.isfinite(out[name]).all(), name
    assert np.abs(out["U"]).max() <= sat
    xs = m4q.plant_rollout_batch(cs.x0, out["U"], cs.op0, cs.ops, cs.ts, cs.kind, u_scale=cs.u_scale)["xs"]
    assert _bits(xs, out["X"])
    print("%s %s %s: status %s, alpha %s, cost %s; %s" % (cs.id, method, "exact" if exact else "clipped", out["status"].tolist(),
                                                          out["alpha_hist"][:, 0].tolist(), out["cost"].tolist(), _s_note(cs)))
    for b in cs.quiet:
        x0, us, op0, ops, sc, _ = cs.alone(b)
        alone = call(x0, us, op0, ops, cs.ts, X_bm[b] if cs.per else X_bm, us.reshape(cs.N, cs.m), Q, R, sat, iters=1, steps=4, kind=cs.kind,
                     u_scale=sc, exact=exact)
        for name in ("X", "U", "cost", "cost_hist", "alpha_hist", "n_iter", "status"):
            assert _bits(alone[name][0], out[name][b]), name


# ---------------------------------------------------------------- the multi rollout
def _figure_of(figure):
    return "last" if figure == "last" else "all"


@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("key", NOT_GEN, ids=NOT_GEN_IDS)
def test_plant_rollout_multi(key, figure):
    """Shared sequence (or B = 1): the case's own run, J against the truth.  Per-member sequences: the five sequences go in as S = 5
    shared ones against per-member operators; J[b, b] is the case's run and is held to the truth, every column to the rollout."""
    cs = sd.case(*key)
    tr = sd.truth(cs)
    want = tr["q"][:, cs.N] if figure == "last" else tr["J_sum"]
    seqs = cs.us.reshape(-1, cs.N, cs.m)
    out = m4q.plant_rollout_multi_batch(cs.x0, seqs, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, u_scale=cs.u_scale, figure=figure)
    assert out["J"].shape == (cs.B, seqs.shape[0]) and np.isfinite(out["J"]).all()
    for s in range(seqs.shape[0]):
        roll = m4q.plant_rollout_batch(cs.x0, seqs[s], cs.op0, cs.ops, cs.ts, cs.kind, u_scale=cs.u_scale, W=cs.W, target=cs.f, keep="none",
                                       figure=_figure_of(figure))
        assert _bits(out["J"][:, s], _objectives(roll["q"]))
    assert _bits(out["F"], m4q.ordered_weighted_sum(out["J"]))
    own = np.diagonal(out["J"]) if seqs.shape[0] == cs.B and cs.B > 1 else out["J"][:, 0]
    ref = m4q.plant_rollout_grad_reference(cs.x0, cs.us, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, u_scale=cs.u_scale, figure=figure)
    err, bound = np.abs(own - want).max(), (cs.N + 1 if figure == "sum" else 1) * _figure_bound(cs, tr)
    print("%s %s: J max|dJ| %.2e, definition %.2e, bound %.2e, max|J| = %.3e; %s"
          % (cs.id, figure, err, np.abs(_objectives(ref["q"]) - want).max(), bound, np.abs(want).max(), _s_note(cs)))
    assert err <= bound
    for b in cs.quiet:
        x0, _, op0, ops, sc, f = cs.alone(b)
        alone = m4q.plant_rollout_multi_batch(x0, seqs, op0, ops, cs.ts, cs.W, f, cs.kind, u_scale=sc, figure=figure)
        assert _bits(alone["J"][0], out["J"][b])


@pytest.mark.parametrize("drive", ["nominal", "strong"])
@pytest.mark.parametrize("N", [1, 6])
@pytest.mark.parametrize("cell", sd.HAMILTONIAN + sd.PROCESS)
def test_plant_rollout_multi_with_everything_shared(cell, N, drive):
    """One operator set (stride 0), u_scale=None, one target, S = 3 sequences; N = 1: the next-step prefetch has no next step.
    Against the definition (held to the truth at strong drive by tests/test_strong_drive_host.py) at the gradient family's bound,
    and against plant_rollout_batch bit for bit."""
    cs = sd.case(cell, "shared", 5, N)
    scale = np.array([1.0, 0.3, 0.08])[:, None, None] * (1.0 if drive == "strong" else 1.0 / cs.level)
    seqs = scale * cs.us[None]
    f = cs.f[0]
    for figure in ("last", "sum"):
        out = m4q.plant_rollout_multi_batch(cs.x0, seqs, cs.op0, cs.ops, cs.ts, cs.W, f, cs.kind, figure=figure)
        ref = m4q.plant_rollout_multi_reference(cs.x0, seqs, cs.op0, cs.ops, cs.ts, cs.W, f, cs.kind, figure=figure)
        err = rel(out["J"], ref["J"])
        print("%s N=%d %s %s: J against the definition %.2e over max(1, max|J|), max|J| = %.3e" % (cell, N, drive, figure, err, np.abs(ref["J"]).max()))
        assert err <= TOL and rel(out["F"], ref["F"]) <= TOL
        for s in range(3):
            roll = m4q.plant_rollout_batch(cs.x0, seqs[s], cs.op0, cs.ops, cs.ts, cs.kind, W=cs.W, target=f, keep="none", figure=_figure_of(figure))
            assert _bits(out["J"][:, s], _objectives(roll["q"]))
    if drive == "strong":
        assert max(sd.squarings(sd.norm1(cs.generator(0, t)[0])) for t in range(N)) >= 1       # (u_scale aside, member 0's exponent)


# ---------------------------------------------------------------- a member that is not finite
NAN_CELLS = sd.HAMILTONIAN + sd.PROCESS + sd.GENERATOR
BAD = 2                                                           # a driven member; its control at t = 1 is NaN


@pytest.mark.parametrize("cell", NAN_CELLS)
def test_a_member_that_is_not_finite_leaves_the_others_alone(cell):
    """Per layout, B = 5, N = 6.  The norm of member BAD's exponent at t = 1 is not finite: s = 0, no loop lengthens.  Its outputs
    from there on are NaN; every other member's are the clean run's bits.  (The multi rollout's sequences are shared by the
    ensemble: the NaN sits in sequence BAD of S = 5, every member's J under it is NaN, the other columns are the clean run's.)"""
    cs = sd.case(cell, "per", 5, 6)
    us = cs.us.copy()
    us[BAD, 1, 0] = np.nan
    others = [b for b in range(cs.B) if b != BAD]
    clean = _rollout(cs, keep="all", figure="all")
    out = _rollout(cs, (cs.x0, us, cs.op0, cs.ops, None, cs.f), keep="all", figure="all")
    assert _bits(out["xs"][others], clean["xs"][others]) and _bits(out["q"][others], clean["q"][others])
    assert _bits(out["xs"][BAD, :2], clean["xs"][BAD, :2]) and np.isnan(out["xs"][BAD, 2:]).all() and np.isnan(out["q"][BAD, 2:]).all()
    if sd.is_generator(cell):
        return
    for figure in ("last", "sum"):
        clean = _grad(cs, figure, scale_grad=True)
        out = _grad(cs, figure, (cs.x0, us, cs.op0, cs.ops, None, cs.f), scale_grad=True)
        for name in ("q", "grad", "grad_scale"):
            assert _bits(out[name][others], clean[name][others]), name
        assert np.isnan(out["q"][BAD] if figure == "last" else out["q"][BAD, 2:]).all()
        assert np.isnan(out["grad"][BAD]).all() and np.isnan(out["grad_scale"][BAD]).all()
        clean = m4q.plant_rollout_multi_batch(cs.x0, cs.us, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, figure=figure)
        out = m4q.plant_rollout_multi_batch(cs.x0, us, cs.op0, cs.ops, cs.ts, cs.W, cs.f, cs.kind, figure=figure)
        assert _bits(out["J"][:, others], clean["J"][:, others]) and np.isnan(out["J"][:, BAD]).all()


# ---------------------------------------------------------------- the parameter gradient
PAIRS = sd.all_param_pairs()
PAIR_IDS = [sd.pair_id(*k) for k in PAIRS]


def _param_s_note(pr):
    s = pr.s()["param_block"]
    return "%s; param_block s per member (max over t) %s, member 0 along t %s" % (_s_note(pr.cs), s.max(axis=1).tolist(), s[0].tolist())


def _column_figures(pr):
    """q [B, N + 1]: column t of plant_rollout_batch's figure against column t of the data."""
    cs = pr.cs
    return np.stack([_rollout(cs, (cs.x0, cs.us, cs.op0, cs.ops, cs.u_scale, pr.data[..., t, :]), keep="none", figure="all")["q"][:, t]
                     for t in range(cs.N + 1)], axis=1)


@pytest.mark.parametrize("key", PAIRS, ids=PAIR_IDS)
def test_plant_parameter_gradient(key):
    pr = sd.param_case(*key)
    cs = pr.cs
    tr = sd.param_truth(pr)
    args, kw = pr.args()
    ref = m4q.plant_param_grad_reference(*args, **kw)
    out = m4q.plant_rollout_param_grad_batch(*args, **kw)
    assert set(out) == set(tr)
    for name in sorted(set(tr) - {"J"}):
        err = rel(out[name], tr[name])
        print("%s %s: device %.2e, definition %.2e, over max(1, max|ref|), max|ref| = %.3e" % (pr.id, name, err, rel(ref[name], tr[name]),
                                                                                             np.abs(tr[name]).max()))
        assert out[name].shape == tr[name].shape and np.isfinite(out[name]).all()
        assert err <= TOL
    cw = pr.weights()
    err_J, Jb = np.abs(out["J"] - tr["J"]).max(), cw.sum() * _figure_bound(cs, sd.truth(cs), pr.data)
    print("%s J: max|dJ| %.2e, definition %.2e, bound %.2e, max|J| = %.3e; %s"
          % (pr.id, err_J, np.abs(ref["J"] - tr["J"]).max(), Jb, np.abs(tr["J"]).max(), _param_s_note(pr)))
    assert np.isfinite(out["J"]).all() and err_J <= Jb
    # J is the ordered sum of the rollout's own figures, weighted, each product rounded before it is added
    q = _column_figures(pr)
    J = np.zeros(cs.B)
    for t in range(cs.N + 1):
        if cw[t] != 0.0:
            J = J + cw[t] * q[:, t]
    assert _bits(out["J"], J)
    # the quiet member alone: the same bits - with the gains in the shared layout its block squares and its forward step does not
    for b in cs.quiet:
        a_args, a_kw = pr.alone(b)
        alone = m4q.plant_rollout_param_grad_batch(*a_args, **a_kw)
        assert all(_bits(alone[name][0], out[name][b]) for name in out)


@pytest.mark.parametrize("cell", sd.PARAM_CELLS)
def test_a_member_that_is_not_finite_leaves_the_others_gradients_alone(cell):
    """Per layout, B = 5, N = 6, the cell's last direction set.  Member BAD's control at t = 1 is NaN: its J and its gradients are
    NaN, every other member's outputs are the clean run's bits."""
    pr = sd.param_case(cell, "per", 5, 6, *sd.param_sets(cell)[-1])
    cs = pr.cs
    args, kw = pr.args()
    us = cs.us.copy()
    us[BAD, 1, 0] = np.nan
    others = [b for b in range(cs.B) if b != BAD]
    clean = m4q.plant_rollout_param_grad_batch(*args, **kw)
    out = m4q.plant_rollout_param_grad_batch(args[0], us, *args[2:], **kw)
    assert set(out) == ({"J", "grad_theta", "grad_scale"} if pr.sg else {"J", "grad_theta"})
    for name in out:
        assert np.isfinite(clean[name]).all() and _bits(out[name][others], clean[name][others]), name
        assert np.isnan(out[name][BAD]).all(), name

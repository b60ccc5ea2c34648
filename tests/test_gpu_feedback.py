"""The feedback runs on the device (plant_feedback_kernel, model_feedback_kernel) against their definition (feedback.py) and against
independent steps (the oracle's plant steps, OracleDMDc.predict).  Shapes are the smallest that can go wrong: B = 5 (one full quad
and a ragged one) and B = 1, N in {1, 3, 8} (the prefetch of step t + 1 is clamped at t + 1 < N).

The primary check does not depend on how sensitive a closed loop is: every stored step of ONE free-running launch is held to the
law and to the plant step in NumPy, from the launch's own xs and us (test_*_per_step_residuals).  Measured maxima on an MI355X over
all cases: see DESIGN section 5.9."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from tests import feedback_cases as fc
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests.test_gpu_rollout import _model_chain

pytestmark = pytest.mark.gpu

TOL = 1e-10
MODEL_SHAPES = [(4, 1, 2), (9, 2, 1), (8, 2, 1), (16, 1, 3)]

# law per member or shared, B, N, band, noise kind, u_scale, non-uniform grid
RUNS = [("shared", 5, 8, False, None, False, False), ("per", 5, 8, True, None, True, True), ("shared", 5, 3, True, "iid", True, True),
        ("per", 5, 8, True, "hermitian", False, True), ("per", 1, 1, True, None, False, False), ("shared", 5, 1, False, "iid", True, False),
        ("shared", 1, 8, True, None, True, True)]


# One drive and a shared law leave eight distinct references: seeds picked on the CPU, on the definition's own run, so that both
# bounds and the interior are reached (asserted below, on every run large enough to reach them all)
RESEED = {((4, 1, 2), 0): 1, ((16, 1, 3), 0): 3}


def _noise(kind, rng, B, hermitian_ok=True):
    """Per-member sigma (one member noise-free) and a member base beyond 2^32."""
    if kind is None:
        return None
    if kind == "hermitian" and not hermitian_ok:
        kind = "iid"
    sigma = 0.03 * rng.uniform(0.5, 1.5, B)
    sigma[0] = 0.0
    return m4q.MeasurementNoise(sigma, 4242, kind, member_base=(1 << 32) + 17)


def _check_residuals(law, step, out, x0, sc, noise, expect_all, label, record_property):
    """(a) every stored control against the law in NumPy on the stored state, (b) every stored state against the step from the
    stored state before under the stored control (and the noise of its column); (c) the maxima, printed and recorded."""
    xs, us = out["xs"], out["us"]
    B, N = us.shape[:2]
    assert np.array_equal(xs[:, 0].view(np.float64), x0.view(np.float64))                 # column 0 is x0 bit for bit
    u, s, lo, hi, mag = fc.law_terms(law, xs, us)
    act = fc.activity(law, u, s, lo, hi)
    if expect_all:            # (asserted on the definition's own run by the caller as well: here on what the device did)
        assert act["lower"] > 0 and act["upper"] > 0 and act["interior"] > 0 and (law.du is None or act["band"] > 0), act
    err_u = np.abs(us - u) / np.maximum(1.0, mag)
    res = fc.step_residuals(step, xs, us, sc, noise)
    err_x = np.abs(res).max(axis=2) / np.maximum(1.0, np.abs(xs[:, 1:]).max(axis=2))
    print("%s: max law residual %.2e, max step residual %.2e (relative), bounds active %s" % (label, err_u.max(), err_x.max(), act))
    record_property("max_law_residual", float(err_u.max()))
    record_property("max_step_residual", float(err_x.max()))
    assert err_u.max() <= TOL
    assert err_x.max() <= TOL
    assert np.array_equal(out["status"], np.zeros(B, np.int32))
    near = np.minimum(np.abs(s - lo), np.abs(s - hi)).min(axis=(1, 2)) < 1e-9
    count = ((s <= lo) | (s >= hi)).sum(axis=(1, 2))
    assert np.array_equal(out["clipped"][~near], count[~near])


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "-".join(str(v) for v in r))
@pytest.mark.parametrize("name", fc.PLANTS)
def test_plant_per_step_residuals(name, run, record_property):
    variant, B, N, band, nkind, scaled, grid = run
    c = fc.case(name)
    rng = np.random.default_rng(9500 + 31 * fc.PLANTS.index(name) + 7 * RUNS.index(run))
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    if c.exp is not None:
        ops = np.stack([c.ops] * B)
    ts = fc._grid(rng, N, c.dt) if grid else np.arange(N + 1) * c.dt
    sc = 1 + 0.1 * rng.standard_normal((B, c.m)) if scaled else None
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0], members=B if variant == "per" else None, band=band)
    noise = _noise(nkind, rng, B, c.kind != _lib.PLANT_PROCESS)
    ones = np.ones((B, c.m)) if sc is None else sc
    big = B * N * c.m >= 40
    if big:       # the definition's own run reaches both bounds, the interior and (with one) the band
        ref = m4q.plant_feedback_reference(x0, law, op0, ops, ts, c.kind, u_scale=sc, noise=noise)
        act = fc.activity(law, *fc.law_terms(law, ref["xs"], ref["us"])[:4])
        assert act["lower"] > 0 and act["upper"] > 0 and act["interior"] > 0 and (not band or act["band"] > 0), act
    out = m4q.plant_feedback_batch(x0, law, op0, ops, ts, c.kind, u_scale=sc, noise=noise)
    assert set(out) == {"xs", "us", "clipped", "status"} and out["xs"].shape == (B, N + 1, c.n) and out["us"].shape == (B, N, c.m)
    dts = np.diff(ts)
    _check_residuals(law, lambda b, t, x, v: c.step(x, v, op0[b], list(ops[b]), dts[t]), out, x0, ones, noise, big,
                     "%s %s" % (name, run), record_property)


@pytest.mark.parametrize("run", RUNS[:4] + RUNS[4:5], ids=lambda r: "-".join(str(v) for v in r))
@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_model_per_step_residuals(shape, run, record_property):
    variant, B, N, band, nkind, scaled, _ = run
    n, m, order = shape
    p = kv.scenario(n, m, order)
    rng = np.random.default_rng(9600 + 100 * n + 10 * m + order + 7 * RUNS.index(run) + 1000 * RESEED.get((shape, RUNS.index(run)), 0))
    sat = p["sat"] / kv.TUNING[(n, m)][1]
    x0 = np.ascontiguousarray(p["x0"][:B])
    models = np.ascontiguousarray(p["models"][:B]) if variant == "per" else p["models"][0]
    sc = 1 + 0.1 * rng.standard_normal((B, m)) if scaled else None
    law = fc.make_law(rng, n, m, N, sat, x0[0], members=B if variant == "per" else None, band=band)
    noise = _noise(nkind, rng, B, n != 8)
    ones = np.ones((B, m)) if sc is None else sc
    big = B * N * m >= 40
    if big:
        ref = m4q.model_feedback_reference(x0, law, models, order, u_scale=sc, noise=noise)
        act = fc.activity(law, *fc.law_terms(law, ref["xs"], ref["us"])[:4])
        assert act["lower"] > 0 and act["upper"] > 0 and act["interior"] > 0 and (not band or act["band"] > 0), act
    out = m4q.model_feedback_batch(x0, law, models, order, u_scale=sc, noise=noise)
    md = models if variant == "per" else np.stack([models] * B)
    _check_residuals(law, lambda b, t, x, v: _model_chain(md[b], m, order, x, v[None])[1], out, x0, ones, noise, big,
                     "model %s %s" % (shape, run), record_property)


# ---------------------------------------------------------------- free-running against the definition
def _envelope(define, x0):
    """The definition's run and what it moves by when x0 is scaled by 1 +- 1e-14 (DESIGN sections 2 and 3), per output."""
    ref = define(x0)
    env = {k: 0.0 for k in ("xs", "us", "q")}
    margin = np.full(x0.shape[0], np.inf)
    for eps in (0.0, 1e-14, -1e-14):
        alt = ref if eps == 0.0 else define(x0 * (1 + eps))
        for k in env:
            env[k] = max(env[k], float(np.abs(alt[k] - ref[k]).max()))
        margin = np.minimum(margin, alt["margin"])
    return ref, env, margin


def _against_definition(run, define, x0, label, record_property):
    ref, env, margin = _envelope(define, x0)
    out = run(x0)
    for k in ("xs", "us", "q"):
        err = float(np.abs(out[k] - ref[k]).max())
        bound = TOL * max(1.0, float(np.abs(ref[k]).max())) + 100 * env[k]
        print("%s %s: error %.2e, envelope %.2e, bound %.2e" % (label, k, err, env[k], bound))
        record_property("%s_error" % k, err)
        record_property("%s_envelope" % k, env[k])
        assert err <= bound
    sure = margin >= 1e-9
    assert sure.any() and np.array_equal(out["clipped"][sure], ref["clipped"][sure])
    assert np.array_equal(out["status"], ref["status"])


def _with_margin(law, ref):
    _, s, lo, hi, _ = fc.law_terms(law, ref["xs"], ref["us"])
    ref["margin"] = np.minimum(np.abs(s - lo), np.abs(s - hi)).min(axis=(1, 2))
    return ref


@pytest.mark.parametrize("name", fc.PLANTS)
def test_plant_feedback_against_the_definition(name, record_property):
    c = fc.case(name)
    B, N = 5, 8
    rng = np.random.default_rng(9700 + fc.PLANTS.index(name))
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    if c.exp is not None:
        ops = np.stack([c.ops] * B)
    ts = fc._grid(rng, N, c.dt)
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0], members=B)
    W, f = gc.weights_and_targets(rng, c.n, B)
    noise = _noise("hermitian", rng, B, c.kind != _lib.PLANT_PROCESS)
    kw = dict(u_scale=sc, noise=noise, W=W, target=f, figure="all")
    _against_definition(lambda x: m4q.plant_feedback_batch(x, law, op0, ops, ts, c.kind, **kw),
                        lambda x: _with_margin(law, m4q.plant_feedback_reference(x, law, op0, ops, ts, c.kind, **kw)), x0, name,
                        record_property)


@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_model_feedback_against_the_definition(shape, record_property):
    n, m, order = shape
    p = kv.scenario(n, m, order)
    B, N = 5, 8
    rng = np.random.default_rng(9800 + 100 * n + 10 * m + order)
    sat = p["sat"] / kv.TUNING[(n, m)][1]
    x0, models = np.ascontiguousarray(p["x0"]), p["models"]
    law = fc.make_law(rng, n, m, N, sat, x0[0])
    W, f = gc.weights_and_targets(rng, n, B)
    kw = dict(u_scale=1 + 0.1 * rng.standard_normal((B, m)), noise=_noise("iid", rng, B), W=W, target=f, figure="all")
    _against_definition(lambda x: m4q.model_feedback_batch(x, law, models, order, **kw),
                        lambda x: _with_margin(law, m4q.model_feedback_reference(x, law, models, order, **kw)), x0, "model %s" % (shape,),
                        record_property)


# ---------------------------------------------------------------- bit for bit
def _options_agree(run, rollout, law, N):
    """run(keep, figure, controls) -> dict: every option against the full run, and (a law that commands u_ref whatever the state)
    against the open-loop rollout of u_ref, bit for bit."""
    full = run("all", "all", True)
    xs, q = full["xs"], full["q"]
    for keep in ("none", "last", "all"):
        for figure in ("none", "last", "all"):
            for controls in (False, True):
                out = run(keep, figure, controls)
                want = {"clipped", "status"} | ({"xs"} if keep != "none" else set()) | ({"q"} if figure != "none" else set()) | \
                    ({"us"} if controls else set())
                assert set(out) == want
                if keep != "none":
                    assert np.array_equal(out["xs"].view(np.float64), (xs if keep == "all" else xs[:, N]).view(np.float64))
                if figure != "none":
                    assert np.array_equal(out["q"], q if figure == "all" else q[:, N])
                if controls:
                    assert np.array_equal(out["us"], full["us"])
                assert np.array_equal(out["clipped"], full["clipped"]) and np.array_equal(out["status"], full["status"])
                if rollout is not None and (keep, figure) != ("none", "none"):
                    open_loop = rollout(keep, figure)
                    for k in open_loop:
                        assert np.array_equal(out[k].view(np.float64), open_loop[k].view(np.float64)), (keep, figure, k)
    return full


def _open_law(rng, n, m, N, sat, members=None):
    """Zero gains, no box, no band: the law commands u_ref."""
    lead = () if members is None else (members,)
    return m4q.FeedbackLaw(np.zeros(lead + (N, n + 1, m)), rng.standard_normal(lead + (N, n)), rng.uniform(-sat, sat, lead + (N, m)), np.inf)


@pytest.mark.parametrize("name", ["9-2-hamiltonian", "9-2-generator", "16-1-process", "16-2-hamiltonian"])
def test_plant_feedback_with_zero_gains_is_the_rollout_bitwise(name):
    c = fc.case(name)
    B, N = 5, 3
    rng = np.random.default_rng(9900 + fc.PLANTS.index(name))
    x0 = c.states(rng, B)
    op0, _ = c.member_ops(rng, B)
    ts = fc._grid(rng, N, c.dt)
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    W, f = gc.weights_and_targets(rng, c.n, B)
    for members in (None, B):
        law = _open_law(rng, c.n, c.m, N, c.sat, members)
        full = _options_agree(
            lambda keep, figure, controls: m4q.plant_feedback_batch(x0, law, op0, c.ops, ts, c.kind, u_scale=sc, W=W, target=f, keep=keep,
                                                                    figure=figure, controls=controls),
            lambda keep, figure: m4q.plant_rollout_batch(x0, law.u_ref, op0, c.ops, ts, c.kind, u_scale=sc, W=W, target=f, keep=keep,
                                                         figure=figure), law, N)
        assert np.array_equal(full["us"], np.broadcast_to(law.u_ref, (B, N, c.m)))
        assert np.array_equal(full["clipped"], np.zeros(B, np.int32))


@pytest.mark.parametrize("shape", [(9, 2, 1), (8, 2, 1)], ids=lambda s: "%d-%d-%d" % s)
def test_model_feedback_with_zero_gains_is_the_rollout_bitwise(shape):
    n, m, order = shape
    p = kv.scenario(n, m, order)
    B, N = 5, 3
    rng = np.random.default_rng(9950 + n)
    sat = p["sat"] / kv.TUNING[(n, m)][1]
    x0, models = np.ascontiguousarray(p["x0"]), p["models"]
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    W, f = gc.weights_and_targets(rng, n, B)
    law = _open_law(rng, n, m, N, sat, B)
    full = _options_agree(
        lambda keep, figure, controls: m4q.model_feedback_batch(x0, law, models, order, u_scale=sc, W=W, target=f, keep=keep, figure=figure,
                                                                controls=controls),
        lambda keep, figure: m4q.model_rollout_batch(x0, law.u_ref, models, order, u_scale=sc, W=W, target=f, keep=keep, figure=figure),
        law, N)
    assert np.array_equal(full["us"], law.u_ref)


def test_options_agree_with_an_active_law_and_noise():
    c = fc.case("9-2-hamiltonian")
    B, N = 5, 8
    rng = np.random.default_rng(9960)
    x0 = c.states(rng, B)
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0], members=B)
    W, f = gc.weights_and_targets(rng, c.n, B)
    noise = _noise("hermitian", rng, B)
    full = _options_agree(lambda keep, figure, controls: m4q.plant_feedback_batch(x0, law, c.op0, c.ops, c.dt, c.kind, noise=noise, W=W,
                                                                                  target=f, keep=keep, figure=figure, controls=controls),
                          None, law, N)
    assert full["clipped"].min() > 0
    # sigma = 0 adds (+0, +0) to every entry: the values of a noise-free run (only the sign of a zero could differ)
    quiet = m4q.plant_feedback_batch(x0, law, c.op0, c.ops, c.dt, c.kind, noise=m4q.MeasurementNoise(0.0, 4242, "iid"))
    free = m4q.plant_feedback_batch(x0, law, c.op0, c.ops, c.dt, c.kind)
    for k in ("xs", "us", "clipped"):
        assert np.array_equal(quiet[k], free[k])
    assert np.array_equal(full["xs"][0], free["xs"][0]) and not np.array_equal(full["xs"][1], free["xs"][1])      # (sigma[0] = 0)


def test_member_does_not_depend_on_its_place():
    """Five members, each with its own law, operators, scales and targets: alone (B = 1) and at four places among 261 members
    (65 quads and a ragged one) they give the same bits."""
    c = fc.case("9-2-hamiltonian")
    N, B = 3, 261
    rng = np.random.default_rng(9970)
    x5 = c.states(rng, 5)
    op5, ops5 = c.member_ops(rng, 5)
    sc5 = 1 + 0.1 * rng.standard_normal((5, c.m))
    law5 = fc.make_law(rng, c.n, c.m, N, c.sat, x5[0], members=5)
    W, f5 = gc.weights_and_targets(rng, c.n, 5)
    ts = fc._grid(rng, N, c.dt)
    idx = np.arange(B) % 5
    law = m4q.FeedbackLaw(law5.gains[idx], law5.x_ref[idx], law5.u_ref[idx], law5.sat, law5.du, law5.u_prev[idx])
    full = m4q.plant_feedback_batch(x5[idx], law, op5[idx], ops5[idx], ts, c.kind, u_scale=sc5[idx], W=W, target=f5[idx], figure="all")
    assert np.array_equal(full["status"], np.zeros(B, np.int32))
    for i in range(5):
        one_law = m4q.FeedbackLaw(law5.gains[i], law5.x_ref[i], law5.u_ref[i], law5.sat, law5.du, law5.u_prev[i])
        one = m4q.plant_feedback_batch(x5[i:i + 1], one_law, op5[i], ops5[i], ts, c.kind, u_scale=sc5[i:i + 1], W=W, target=f5[i:i + 1],
                                       figure="all")
        for place in (i, i + 65, i + 130, i + 255):
            for k in ("xs", "q", "us", "clipped"):
                assert np.array_equal(one[k][0].view(np.float64) if k != "clipped" else one[k][0],
                                      full[k][place].view(np.float64) if k != "clipped" else full[k][place]), (i, place, k)
    assert len({full["xs"][b].tobytes() for b in range(5)}) == 5                        # (the members do differ)


# ---------------------------------------------------------------- the law's convention
@pytest.mark.parametrize("shape,T", [((4, 1, 1), 6), ((9, 2, 1), 8)], ids=["4-1-1", "9-2-1"])
def test_law_of_a_quad_program_reproduces_its_solution(shape, T):
    """gains, X_opt, U_opt of one quad_program_batch with bounds active on some indices (no u_prev): the NumPy rollout of
    FeedbackLaw.from_quad_program on the QP's own A_ls, B_ls, Delta_ls gives X_opt and U_opt back to 1e-10."""
    n, m, order = shape
    p = kv.scenario(n, m, order)
    B = 3
    rng = np.random.default_rng(9980 + n)
    x0 = np.ascontiguousarray(p["x0"][:B])
    wm = m4q.WrapModel(p["models"][0][:, :n], p["models"][0][:, n:], m, order)
    Xg = np.repeat(x0[:, None, :], T, axis=1)
    Ug = 0.3 * p["sat"] * rng.standard_normal((B, T, m))
    A_ls, B_ls, D_ls = wm.linearize_batch(Xg, Ug)
    X_bm = np.ascontiguousarray(np.asarray(p["X_targ"]).T[None, :T + 1])
    U_bm = 0.2 * p["sat"] * rng.standard_normal((1, T, m))
    Q_ls = np.stack([np.asarray(p["Q"], complex)] * T + [np.asarray(p["Qf"], complex)])
    R_ls = np.stack([np.asarray(p["R"], complex) / kv.TUNING[(n, m)][0] * 1e-2] * T)
    _, U_free, _, _ = m4q.quad_program_batch(x0, X_bm, U_bm, Q_ls, R_ls, A_ls, B_ls, D_ls, sat=1e6)
    sat = 0.5 * np.abs(U_free).max()
    X_opt, U_opt, _, gains = m4q.quad_program_batch(x0, X_bm, U_bm, Q_ls, R_ls, A_ls, B_ls, D_ls, sat=sat)
    active = np.abs(U_opt) >= sat
    assert 0 < active.sum() < active.size
    law = m4q.FeedbackLaw.from_quad_program(gains, X_bm, U_bm, sat)
    assert law.members == B and law.N == T
    for b in range(B):
        x = x0[b]
        for t in range(T):
            assert np.abs(x - X_opt[b, t]).max() <= 1e-10
            u = law.control(t, x, member=b)
            assert np.abs(u - U_opt[b, t]).max() <= 1e-10
            x = A_ls[b, t] @ x + B_ls[b, t] @ u + D_ls[b, t]
        assert np.abs(x - X_opt[b, T]).max() <= 1e-10


# ---------------------------------------------------------------- status
@pytest.mark.parametrize("model", [False, True], ids=["plant", "model"])
def test_a_lost_member_is_reported_and_its_neighbours_keep_their_bits(model):
    c = fc.case("9-2-hamiltonian")
    B, N = 5, 3
    rng = np.random.default_rng(9990)
    x0 = c.states(rng, B)
    law = fc.make_law(rng, c.n, c.m, N, c.sat, x0[0], members=B)
    if model:
        models = kv.scenario(9, 2, 1)["models"]
        run = lambda x: m4q.model_feedback_batch(x, law, models, 1)            # noqa: E731
    else:
        run = lambda x: m4q.plant_feedback_batch(x, law, c.op0, c.ops, c.dt, c.kind)      # noqa: E731
    good = run(x0)
    bad0 = x0.copy()
    bad0[2, 4] = np.nan
    got = run(bad0)
    assert np.array_equal(good["status"], np.zeros(B, np.int32)) and np.array_equal(got["status"], [0, 0, 3, 0, 0])
    for b in (0, 1, 3, 4):
        for k in ("xs", "us"):
            assert np.array_equal(got[k][b].view(np.float64), good[k][b].view(np.float64))
        assert got["clipped"][b] == good["clipped"][b]


# ---------------------------------------------------------------- the experiments' entry points
def test_feedback_batch_follows_plant_feedback_batch():
    rng = np.random.default_rng(9995)
    ts = np.array([0.0, 0.2, 0.5, 0.55])
    for name in ("9-2-hamiltonian", "9-2-generator"):
        c = fc.case(name)
        exp = c.exp if c.exp is not None else m4q.QExperiment(c.op0, list(c.ops))
        x0 = c.states(rng, 3)
        law = fc.make_law(rng, c.n, c.m, 3, c.sat, x0[0])
        noise = m4q.MeasurementNoise(0.01, 5, "hermitian")
        sc = 1 + 0.1 * rng.standard_normal((3, c.m))
        got = exp.feedback_batch(x0, ts, law, u_scale=sc, noise=noise)
        own0, ops = exp.operators()
        want = m4q.plant_feedback_batch(x0, law, own0, ops, ts, exp.plant_kind, u_scale=sc, noise=noise)
        assert exp.plant_kind == c.kind and set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k])
        assert exp.xs is None and exp.ts is None
    syn = m4q.QSynthesis(0.15 * configs.SZ, [0.5 * configs.SX])
    c = fc.case("16-1-process")
    x0 = c.states(rng, 3)
    law = fc.make_law(rng, 16, 1, 3, c.sat, x0[0])
    got = syn.feedback_batch(x0, ts, law, keep="last")
    want = m4q.plant_feedback_batch(x0, law, *syn.operators(), ts, _lib.PLANT_PROCESS, keep="last")
    assert np.array_equal(got["xs"], want["xs"]) and np.array_equal(got["us"], want["us"])


def test_along_trajectory_tracks_its_own_nominal_trajectory(record_property):
    """Only a shape-and-plumbing check: a law built around the model's own rollout, with that rollout as the QP's benchmark, has
    the nominal controls as its optimum, so the feedback run from the nominal x0 on the model it was designed on retraces the
    nominal trajectory - to the envelope of that rollout (what it moves by when x0 is scaled by 1 +- 1e-14)."""
    p = configs.build(1)
    n, m, N = 4, 1, 12
    rng = np.random.default_rng(9999)
    model = np.asarray(p["models"][0])
    x0 = np.ascontiguousarray(p["x0"][:1])
    U_nom = rng.uniform(-0.5 * p["sat"], 0.5 * p["sat"], (N, m))
    X_nom = m4q.model_rollout_batch(x0, U_nom, model, 1)["xs"][0]
    law = m4q.FeedbackLaw.along_trajectory(model, 1, X_nom, U_nom, X_nom, U_nom, np.asarray(p["Q"]), np.asarray(p["R"]), p["sat"])
    assert law.N == N and law.n == n and law.m == m and law.members is None and np.abs(law.gains[:, :n]).max() > 0
    out = m4q.model_feedback_batch(x0, law, model, 1)
    env = max(np.abs(m4q.model_rollout_batch(x0 * (1 + e), U_nom, model, 1)["xs"][0] - X_nom).max() for e in (1e-14, -1e-14))
    err = np.abs(out["xs"][0] - X_nom).max()
    print("along_trajectory: error %.2e, envelope %.2e" % (err, env))
    record_property("error", float(err))
    record_property("envelope", float(env))
    assert err <= TOL * max(1.0, np.abs(X_nom).max()) + 100 * env
    assert np.abs(out["us"][0] - U_nom).max() <= TOL * max(1.0, np.abs(law.gains).sum(axis=(1, 2)).max()) + 100 * env
    assert out["status"][0] == 0

"""Every auxiliary kernel the library holds, run once per compiled instance: one test id per cell of kernel_variants.aux_cells() -
the rollouts, gradients, stored feedback laws, plant linearisation, the four DMDc fits and the online update at every (dim_x, dim_u,
order) object and plant kind that builds them - and every kernel's second trip through its grid-stride loop.

Inputs are tests/aux_matrix_cases.py's (B = 5: one full wavefront and one more row; shared and per-member operands), whose
preconditions tests/test_aux_matrix_host.py holds on the CPU.  Every cell is compared with its family's definition at the bound the
family's own test file uses - the constant or the function is imported from there, nothing is chosen here:

  model / plant rollout    gc.model_chain / gc.plant_chain                      TOL of tests/test_gpu_rollout.py
  model / plant gradient   model_ / plant_rollout_grad_reference, both figures  _compare of tests/test_gpu_grad.py
  model / plant feedback   model_ / plant_feedback_reference                    _check_residuals, _against_definition of tests/test_gpu_feedback.py
  fit, fit_qr, refit(_qr)  NumPy's pinv for all members, the route's definition status_ok, check, ROUTES of tests/test_gpu_refit.py
  online, both forms       online.online_dmdc_reference, E = 1 and 2            against of tests/test_gpu_online.py
  plant linearisation      plant_linearize_reference                            TOL of tests/test_gpu_plant_linearize.py

A refused cell asserts the refusal and its message.  The second-trip tests build an ensemble just past the grid cap from five
distinct members and hold each member alone (B = 1) to its copies before and after the wrap, bit for bit."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd.observe import OBSERVE_PARTIAL_TRACE, OBSERVE_QUBIT_BLOCK, observe_batch, observe_dims
from tests import aux_matrix_cases as amc
from tests import feedback_cases as fc
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests.test_gpu_feedback import TOL as FEEDBACK_TOL, _against_definition, _check_residuals
from tests.test_gpu_grad import TOL as GRAD_TOL, _compare as grad_compare
from tests.test_gpu_online import FIELDS as ONLINE_FIELDS, against as online_against, sensitivity
from tests.test_gpu_plant_linearize import NAMES as LIN_NAMES, TOL as LIN_TOL
from tests.test_gpu_refit import ROUTES, check as fit_check, status_ok
from tests.test_gpu_rollout import PICK, TOL as ROLL_TOL
from tests.test_gpu_variant_matrix import _random_ltv
from tests.test_plant_linearize_host import _LinCall

pytestmark = pytest.mark.gpu

CELLS = kv.aux_cells()


def _cells(family):
    return [c for c in CELLS if c.family == family]


class _Worst:
    """Collects error / bound over the comparisons of one cell; record() leaves the largest as the cell's figure (DESIGN section 3's
    table).  tagged(tag) is a record_property for the imported checks: it records under the tag and keeps what they measured."""

    def __init__(self, record_property):
        self.record_property, self.worst, self.seen = record_property, 0.0, {}

    def add(self, err, bound):
        self.worst = max(self.worst, float(err) / float(bound))

    def tagged(self, tag):
        def rec(key, value):
            self.seen[key] = value
            self.record_property("%s_%s" % (tag, key), value)
        return rec

    def record(self, label):
        print("%s: worst error / bound = %.3g" % (label, self.worst))
        self.record_property("worst_error_over_bound", self.worst)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if np.iscomplexobj(a):
        a, b = np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)
    return a.shape == b.shape and np.array_equal(a, b)


def _refusal(call, code, *words):
    with pytest.raises(_lib.M4qError) as err:
        call()
    assert err.value.code == code, err.value
    assert all(w in str(err.value) for w in words), err.value
    print("refused: %s" % err.value)


# ---------------------------------------------------------------- rollouts
def _rollout_cell(label, case, reference, run, record_property):
    worst = _Worst(record_property)
    for variant in amc.VARIANTS:
        c = case(variant)
        ref = reference(c)
        xs = run(c)["xs"]
        assert xs.shape == ref.shape and _bits(xs[:, 0], c["x0"])                         # column 0 is x0 bit for bit
        err, bound = float(np.abs(xs - ref).max()), ROLL_TOL * max(1.0, float(np.abs(ref).max()))
        print("%s %s: max|dx| = %.3e, bound %.3e" % (label, variant, err, bound))
        record_property(variant + "_error", err)
        record_property(variant + "_bound", bound)
        worst.add(err, bound)
        assert err <= bound
    worst.record(label)


@pytest.mark.parametrize("cell", _cells("model_rollout"), ids=kv.aux_cell_id)
def test_model_rollout_cell(cell, record_property):
    _rollout_cell(kv.aux_cell_id(cell), lambda v: amc.model_rollout_case(cell.nx, cell.nu, cell.order, v), amc.model_rollout_reference,
                  lambda c: m4q.model_rollout_batch(c["x0"], c["u"], c["models"], c["order"], u_scale=c["u_scale"]), record_property)


@pytest.mark.parametrize("cell", _cells("plant_rollout"), ids=kv.aux_cell_id)
def test_plant_rollout_cell(cell, record_property):
    _rollout_cell(kv.aux_cell_id(cell), lambda v: amc.plant_rollout_case(cell.nx, cell.nu, cell.kind, v), amc.plant_rollout_reference,
                  lambda k: m4q.plant_rollout_batch(k["x0"], k["u"], k["op0"], k["ops"], k["ts"], k["c"].kind, u_scale=k["u_scale"]),
                  record_property)


# ---------------------------------------------------------------- gradients
def _grad_cell(label, case, reference, run, roll, record_property):
    worst = _Worst(record_property)
    for variant in amc.VARIANTS:
        c = case(variant)
        for figure in amc.FIGURES:
            ref = reference(c, figure)
            out = run(c, figure)
            assert set(out) == {"q", "grad", "grad_scale"}
            for key in ("grad", "grad_scale"):
                err = float(np.abs(out[key] - ref[key]).max() / max(1.0, np.abs(ref[key]).max()))
                record_property("%s_%s_%s_error" % (variant, figure, key), err)
                worst.add(err, GRAD_TOL)
            grad_compare(out, ref, "%s %s %s (bound %.1e)" % (label, variant, figure, GRAD_TOL))     # (prints and asserts every figure)
            # the forward pass is the rollout's own: the same figure, bit for bit
            assert np.array_equal(out["q"], roll(c, "last" if figure == "last" else "all")["q"])
    worst.record(label)


@pytest.mark.parametrize("cell", _cells("model_grad"), ids=kv.aux_cell_id)
def test_model_gradient_cell(cell, record_property):
    _grad_cell(kv.aux_cell_id(cell), lambda v: amc.model_grad_case(cell.nx, cell.nu, cell.order, v), amc.model_grad_reference,
               lambda c, fig: m4q.model_rollout_grad_batch(c["x0"], c["u"], c["models"], c["order"], c["W"], c["target"], u_scale=c["u_scale"],
                                                           figure=fig, scale_grad=True),
               lambda c, fig: m4q.model_rollout_batch(c["x0"], c["u"], c["models"], c["order"], u_scale=c["u_scale"], W=c["W"],
                                                      target=c["target"], keep="none", figure=fig), record_property)


@pytest.mark.parametrize("cell", _cells("plant_grad"), ids=kv.aux_cell_id)
def test_plant_gradient_cell(cell, record_property):
    if cell.kind == kv.REFUSED:
        c = amc.plant_case(cell.nx, cell.nu, kv.GENERATOR)
        x0 = c.states(np.random.default_rng(1), 2)
        _refusal(lambda: m4q.plant_rollout_grad_batch(x0, np.zeros((3, c.m)), c.op0, c.ops, c.dt, np.eye(c.n), np.zeros(c.n),
                                                      _lib.PLANT_GENERATOR),
                 _lib.E_UNSUPPORTED, "m4q_plant_rollout_grad_batch", "the generator plant has no gradient kernel")
        return
    _grad_cell(kv.aux_cell_id(cell), lambda v: amc.plant_grad_case(cell.nx, cell.nu, cell.kind, v), amc.plant_grad_reference,
               lambda k, fig: m4q.plant_rollout_grad_batch(k["x0"], k["u"], k["op0"], k["ops"], k["ts"], k["W"], k["target"], k["c"].kind,
                                                           u_scale=k["u_scale"], figure=fig, scale_grad=True),
               lambda k, fig: m4q.plant_rollout_batch(k["x0"], k["u"], k["op0"], k["ops"], k["ts"], k["c"].kind, u_scale=k["u_scale"],
                                                      W=k["W"], target=k["target"], keep="none", figure=fig), record_property)


# ---------------------------------------------------------------- feedback
def _feedback_cell(label, case, define, run, step_of, record_property):
    """(The cell's figure is the larger per-step residual over TOL: the primary check of tests/test_gpu_feedback.py.)"""
    worst = _Worst(record_property)
    for variant in amc.VARIANTS:
        c = case(variant)
        out = run(c, c["x0"])
        assert set(out) == {"xs", "us", "q", "clipped", "status"}
        rec = worst.tagged(variant)
        _check_residuals(c["law"], step_of(c), out, c["x0"], c["kw"]["u_scale"], c["kw"]["noise"], True,
                         "%s %s (bound %.1e)" % (label, variant, FEEDBACK_TOL), rec)
        worst.add(max(worst.seen["max_law_residual"], worst.seen["max_step_residual"]), FEEDBACK_TOL)
        _against_definition(lambda x: out, lambda x: define(c, x), c["x0"], "%s %s" % (label, variant), rec)
    worst.record(label)


@pytest.mark.parametrize("cell", _cells("model_feedback"), ids=kv.aux_cell_id)
def test_model_feedback_cell(cell, record_property):
    def step_of(c):
        md = c["models"] if c["models"].ndim == 3 else np.stack([c["models"]] * amc.B)
        return lambda b, t, x, v: gc.model_chain(md[b], c["m"], c["order"], x, v[None])[1]
    _feedback_cell(kv.aux_cell_id(cell), lambda v: amc.model_feedback_case(cell.nx, cell.nu, cell.order, v), amc.model_feedback_define,
                   lambda c, x: m4q.model_feedback_batch(x, c["law"], c["models"], c["order"], **c["kw"]), step_of, record_property)


@pytest.mark.parametrize("cell", _cells("plant_feedback"), ids=kv.aux_cell_id)
def test_plant_feedback_cell(cell, record_property):
    def step_of(k):
        dts = amc.dts_of(k["ts"], amc.N_FEEDBACK)
        return lambda b, t, x, v: k["c"].step(x, v, k["op0"][b], list(k["ops"][b]), dts[t])
    _feedback_cell(kv.aux_cell_id(cell), lambda v: amc.plant_feedback_case(cell.nx, cell.nu, cell.kind, v), amc.plant_feedback_define,
                   lambda k, x: m4q.plant_feedback_batch(x, k["law"], k["op0"], k["ops"], k["ts"], k["c"].kind, **k["kw"]), step_of,
                   record_property)


# ---------------------------------------------------------------- plant linearisation
@pytest.mark.parametrize("cell", _cells("plant_linearize"), ids=kv.aux_cell_id)
def test_plant_linearize_cell(cell, record_property):
    if cell.kind == kv.REFUSED:
        c = amc.plant_case(cell.nx, cell.nu, kv.GENERATOR)
        with pytest.raises(ValueError, match="the generator plant has no linearisation"):
            m4q.plant_linearize_batch(np.zeros((2, 3, c.n), complex), np.zeros((3, c.m)), c.op0, c.ops, c.dt, _lib.PLANT_GENERATOR)
        assert _LinCall(n=c.n, m=c.m, kind=_lib.PLANT_GENERATOR, k=c.n)() == _lib.E_UNSUPPORTED          # the C entry point itself
        msg = _lib.lib().m4q_last_error().decode()
        print("refused: %s" % msg)
        assert "m4q_plant_linearize_batch" in msg and "the generator plant has no linearisation kernel" in msg
        return
    worst = _Worst(record_property)
    for variant in amc.VARIANTS:
        k = amc.plant_linearize_case(cell.nx, cell.nu, cell.kind, variant)
        ref = amc.plant_linearize_reference(k)
        out = m4q.plant_linearize_batch(k["X"], k["U"], k["op0"], k["ops"], k["ts"], k["c"].kind, u_scale=k["u_scale"])
        for what, got, want in zip(LIN_NAMES, out, ref):
            assert got.shape == want.shape and got.dtype == np.complex128 and np.isfinite(got).all()
            err = float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
            print("%s %s: max|d%s| / max(1, max|ref|) = %.3e, bound %.3e" % (kv.aux_cell_id(cell), variant, what, err, LIN_TOL))
            record_property("%s_%s_error" % (variant, what), err)
            worst.add(err, LIN_TOL)
            assert err <= LIN_TOL
    worst.record(kv.aux_cell_id(cell))


# ---------------------------------------------------------------- the four fits
def _unfit_data(order=4, prior=False):
    """Well-formed arguments at (16, 1, 4), nz = 80: what the fit and online entry points refuse for want of a kernel."""
    rng = np.random.default_rng(2)
    args = dict(xs=rng.standard_normal((2, 5, 16)) + 0j, us=rng.standard_normal((4, 1)), order=order)
    if prior:
        args["A0"] = np.zeros((16, 80), dtype=complex)
    return args


@pytest.mark.parametrize("cell", [c for c in CELLS if c.family in kv.FIT_FAMILIES], ids=kv.aux_cell_id)
def test_fit_cell(cell, record_property):
    family, nx, nu, order, kind = cell
    route, prior = ("qr" if family.endswith("qr") else "gram"), family.startswith("refit")
    entry = {"fit": "m4q_dmdc_fit_batch", "fit_qr": "m4q_dmdc_fit_qr_batch", "refit": "m4q_dmdc_refit_batch",
             "refit_qr": "m4q_dmdc_refit_qr_batch"}[family]
    if kind == kv.REFUSED:
        assert (nx, nu) == (16, 1)
        _refusal(lambda: m4q.dmdc_fit_batch(rcond=1e-3, method=route, **_unfit_data(order, prior)), _lib.E_UNSUPPORTED, entry,
                 "nz = %d" % kv.lifted_size(nx, nu, order), "do not fit one workgroup's LDS")
        return
    definition, bounds = ROUTES[route]
    c = amc.fit_case(nx, nu, order, prior)
    name = "%s-%d-%d-%d" % (family, nx, nu, order)
    worst = _Worst(record_property)
    out = m4q.dmdc_fit_batch(method=route, **amc.fit_args(c, prior))
    assert status_ok(out, c, route), out["status"]
    assert np.array_equal(out["rank"], c["rank"])
    fit_check(out["models"], c, bounds, "kernel against NumPy's pinv", name, worst.tagged("pinv"))
    worst.add(worst.seen["worst_error_over_bound"], 1.0)
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    print("%s: max |s - s_ref| / s_0 per member = %s, bound 1e-12" % (name, err))
    record_property("worst_sval_error_over_s0", float(err.max()))
    worst.add(err.max(), 1e-12)
    assert np.all(np.diff(out["svals"], axis=1) <= 0) and np.all(err <= 1e-12)
    # the route's definition, on the first two members where nz >= 48 (a Python loop over rotations)
    k = amc.fit_definition_members(c)
    sub = amc.fit_members(c, k)
    want = definition(**amc.fit_args(sub, prior))
    assert np.array_equal(out["rank"][:, :k], want["rank"]) and status_ok(want, c, route)
    fit_check(out["models"][:, :k], dict(sub, A=want["models"]), bounds, "kernel against its definition", name,
              worst.tagged("definition"))
    worst.add(worst.seen["worst_error_over_bound"], 1.0)
    worst.record(name)


# ---------------------------------------------------------------- online
@pytest.mark.parametrize("cell", _cells("online"), ids=kv.aux_cell_id)
def test_online_cell(cell, record_property):
    if cell.kind == kv.REFUSED:
        for hermitian in (False, True):
            _refusal(lambda: m4q.online_dmdc_batch(alpha=amc.ALPHA, hermitian=hermitian, **_unfit_data(cell.order, True)),
                     _lib.E_UNSUPPORTED, "m4q_online_dmdc_batch", "nz = %d" % kv.lifted_size(cell.nx, cell.nu, cell.order),
                     "does not fit one wavefront")
        return
    hermitian = cell.kind == kv.HERMITIAN_FORM
    args = amc.online_args(cell.nx, cell.nu, cell.order, hermitian)
    want = amc.online_reference(args)
    got = m4q.online_dmdc_batch(**args)
    worst = _Worst(record_property)
    s = sensitivity(args, want)
    online_against(got, want, s, worst.tagged("e1"), kv.aux_cell_id(cell))
    for err, sens in (("err_A", "s_A"), ("err_hist", "s_A"), ("err_P", "s_P"), ("err_innov", "s_innov")):
        bound = max(1e-12, 100 * worst.seen[sens])                                        # against()'s own bound
        print("%s: %s = %.3g, bound %.3g" % (kv.aux_cell_id(cell), err, worst.seen[err], bound))
        worst.add(worst.seen[err], bound)
    worst.record(kv.aux_cell_id(cell))
    cut = m4q.online_dmdc_batch(**amc.online_args(cell.nx, cell.nu, cell.order, hermitian, E=2))
    for f in ONLINE_FIELDS:                               # the trajectory cut in two is the same sequence of updates: bit for bit
        assert np.array_equal(got[f], cut[f]), f


# ---------------------------------------------------------------- the second trip of the grid-stride loops
B_QUAD = PICK[-1] + 1                    # 16,389 members: 4,098 quads, one more than the grid, the last one ragged
B_FIT = kv.AUX_GRID + 3                  # 4,099 members of a kernel that holds one per workgroup


def _places(i, wrap, total):
    """Where member i of five sits among `total` members tiled with arange(total) % 5: its first place, its last place of the first
    trip, its first place of the second trip and its last place of all (the ragged tail) - those of them that exist."""
    own = [p for p in range(total) if p % 5 == i]
    return sorted({own[0], max(p for p in own if p < wrap), min([p for p in own if p >= wrap] or own[:1]), own[-1]})


def _second_trip(run_all, run_one, fields, wrap, total):
    """run_all() -> the ensemble's outputs (dict, member axis first); run_one(i, place) -> member i alone (B = 1)."""
    assert (wrap, total) in ((kv.QUAD_WRAP, B_QUAD), (kv.AUX_GRID, B_FIT))
    if wrap == kv.QUAD_WRAP:
        assert set(PICK) <= {p for i in range(5) for p in _places(i, wrap, total)}
    full = run_all()
    seen = 0
    for i in range(5):
        for place in _places(i, wrap, total):
            one = run_one(i, place)
            for f in fields:
                assert _bits(one[f][0], full[f][place]), (f, i, place)
            seen += place >= wrap
    assert seen >= 3                                                                      # places of the second trip were compared
    for f in fields:
        assert np.all(np.isfinite(full[f][:5]))
    assert len({b"".join(np.ascontiguousarray(full[f][b]).tobytes() for f in fields) for b in range(5)}) == 5   # the members differ


IDX_QUAD, IDX_FIT = np.arange(B_QUAD) % 5, np.arange(B_FIT) % 5


def _fit_second_trip(nx, nu, route, prior):
    c = amc.fit_case(nx, nu, 1, True)
    N = 12
    xs, us = np.ascontiguousarray(c["xs"][:, :1, :N + 1]), np.ascontiguousarray(c["us"][:1, :N])
    sc = 1 + 0.1 * np.random.default_rng(4).standard_normal((5, nu))
    disc, counts = np.array([0.95, 0.9, 1.0, 0.97, 0.8]), np.array([N, 7, N, N - 1, 3], dtype=np.int32)

    def run(idx):
        kw = dict(A0=np.ascontiguousarray(c["A0"][idx]), discount=disc[idx], counts=counts[idx]) if prior else {}
        out = m4q.dmdc_fit_batch(np.ascontiguousarray(xs[idx]), us, 1, c["rconds"], u_scale=np.ascontiguousarray(sc[idx]), method=route, **kw)
        assert np.all(out["status"] <= 1)
        return dict(models=np.moveaxis(out["models"], 1, 0), rank=np.moveaxis(out["rank"], 1, 0), svals=out["svals"], status=out["status"])
    _second_trip(lambda: run(IDX_FIT), lambda i, place: run(np.array([i])), ("models", "rank", "svals", "status"), kv.AUX_GRID, B_FIT)


@pytest.mark.parametrize("shape", [(4, 1), (9, 2)], ids=["4-1-1", "9-2-1"])
def test_dmdc_fit_second_trip(shape):
    _fit_second_trip(*shape, "gram", False)


@pytest.mark.parametrize("shape", [(4, 1), (9, 2)], ids=["4-1-1", "9-2-1"])
def test_dmdc_fit_qr_second_trip(shape):
    _fit_second_trip(*shape, "qr", False)


@pytest.mark.parametrize("shape", [(4, 1), (9, 2)], ids=["4-1-1", "9-2-1"])
def test_dmdc_refit_second_trip(shape):
    _fit_second_trip(*shape, "gram", True)


@pytest.mark.parametrize("shape", [(4, 1), (9, 2)], ids=["4-1-1", "9-2-1"])
def test_dmdc_refit_qr_second_trip(shape):
    _fit_second_trip(*shape, "qr", True)


def _feedback_five(rng, n, m, N, sat, x5):
    """Five members' own laws (with u_prev), scales, targets and noise levels."""
    law5 = fc.make_law(rng, n, m, N, sat, x5[0], members=5)
    W, f5 = gc.weights_and_targets(rng, n, 5)
    return law5, 1 + 0.1 * rng.standard_normal((5, m)), W, f5, 0.03 * rng.uniform(0.5, 1.5, 5)


def _law_of(law5, idx):
    return m4q.FeedbackLaw(law5.gains[idx], law5.x_ref[idx], law5.u_ref[idx], law5.sat, law5.du, law5.u_prev[idx])


def _feedback_second_trip(run, x5, law5, sc5, W, f5, sigma5):
    """run(x0, law, idx, **kw): the members idx of the five.  The noise of a member is drawn at its place (member_base + row), so
    the member alone is given its place as the base."""
    base = (1 << 32) + 17

    def call(idx, member_base):
        noise = m4q.MeasurementNoise(sigma5[idx], 4242, "hermitian", member_base=member_base)
        out = run(np.ascontiguousarray(x5[idx]), _law_of(law5, idx), idx, u_scale=np.ascontiguousarray(sc5[idx]), noise=noise, W=W,
                  target=np.ascontiguousarray(f5[idx]), figure="all")
        assert np.array_equal(out["status"], np.zeros(len(idx), np.int32))
        return out
    _second_trip(lambda: call(IDX_QUAD, base), lambda i, place: call(np.array([i]), base + place), ("xs", "q", "us", "clipped", "status"),
                 kv.QUAD_WRAP, B_QUAD)


def test_model_feedback_second_trip():
    p = kv.scenario(4, 1, 1)
    rng = np.random.default_rng(9971)
    x5, models5 = np.ascontiguousarray(p["x0"]), np.ascontiguousarray(p["models"])
    five = _feedback_five(rng, 4, 1, 3, amc.model_sat(p), x5)
    _feedback_second_trip(lambda x0, law, idx, **kw: m4q.model_feedback_batch(x0, law, np.ascontiguousarray(models5[idx]), 1, **kw), x5, *five)


def test_plant_feedback_second_trip():
    c = amc.plant_case(4, 1, kv.HAMILTONIAN)
    rng = np.random.default_rng(9972)
    x5 = c.states(rng, 5)
    op5, ops5 = c.member_ops(rng, 5)
    ts = gc.grid(rng, 3, c.dt)
    five = _feedback_five(rng, 4, 1, 3, c.sat, x5)
    _feedback_second_trip(lambda x0, law, idx, **kw: m4q.plant_feedback_batch(x0, law, np.ascontiguousarray(op5[idx]),
                                                                              np.ascontiguousarray(ops5[idx]), ts, c.kind, **kw), x5, *five)


def test_plant_linearize_second_trip():
    """The quads are of (member, point) pairs: B = 5,463 members of T = 3 points make the 16,389 pairs."""
    c = amc.plant_case(4, 1, kv.HAMILTONIAN)
    rng = np.random.default_rng(9973)
    T = 3
    assert B_QUAD % T == 0
    Bm = B_QUAD // T
    X5 = c.states(rng, 5 * T).reshape(5, T, c.n)
    X5 = X5 + 0.05 * (rng.standard_normal(X5.shape) + 1j * rng.standard_normal(X5.shape))
    U5 = rng.uniform(-c.sat, c.sat, (5, T, c.m))
    op5, ops5 = c.member_ops(rng, 5)
    sc5 = 1 + 0.1 * rng.standard_normal((5, c.m))
    ts = gc.grid(rng, T, c.dt)

    def run(idx):
        return dict(zip(LIN_NAMES, m4q.plant_linearize_batch(X5[idx], U5[idx], op5[idx], ops5[idx], ts, c.kind, u_scale=sc5[idx])))
    idx = np.arange(Bm) % 5
    full = run(idx)
    pairs = {name: a.reshape((Bm * T,) + a.shape[2:]) for name, a in full.items()}        # pair p = (member p // T, point p % T)
    seen = 0
    for i in range(5):
        one = run(np.array([i]))
        own = [b for b in range(Bm) if b % 5 == i]
        past = [b for b in own if (b + 1) * T > kv.QUAD_WRAP]                             # members with a pair of the second trip
        for b in sorted({own[0], max(b for b in own if (b + 1) * T <= kv.QUAD_WRAP), own[-1]} | set(past[:1])):
            for name in LIN_NAMES:
                for t in range(T):
                    assert _bits(one[name][0, t], pairs[name][b * T + t]), (name, i, b, t)
            seen += (b + 1) * T > kv.QUAD_WRAP
    assert seen == 2 and all(np.isfinite(a).all() for a in full.values())        # (members 5,461 and 5,462 hold the five pairs past the wrap)
    assert len({full["B"][b].tobytes() for b in range(5)}) == 5


def test_linearize_second_trip():
    p = kv.scenario(4, 1, 1)
    rng = np.random.default_rng(9974)
    n, m, T = 4, 1, 3
    models5 = np.ascontiguousarray(p["models"])
    X5 = rng.standard_normal((5, T, n)) + 1j * rng.standard_normal((5, T, n))
    U5 = rng.uniform(-1.2, 1.2, (5, T, m))

    def run(idx):
        Bn = len(idx)
        A, Bm, D = np.empty((Bn, T, n, n), complex), np.empty((Bn, T, n, m), complex), np.empty((Bn, T, n), complex)
        _lib.check(_lib.lib().m4q_linearize_batch(Bn, n, m, 1, T, _lib.cbuf(models5[idx])[1], 1, _lib.cbuf(X5[idx])[1], _lib.rbuf(U5[idx])[1],
                                                  A.ctypes.data_as(_lib._dp), Bm.ctypes.data_as(_lib._dp), D.ctypes.data_as(_lib._dp)))
        return dict(A=A, B=Bm, Delta=D)
    _second_trip(lambda: run(IDX_QUAD), lambda i, place: run(np.array([i])), LIN_NAMES, kv.QUAD_WRAP, B_QUAD)


def test_qp_second_trip():
    """Mode qp (no band, no reference LQR, the clipped solve) with the bound active."""
    rng = np.random.default_rng(9975)
    A, Bm, D, x0, Xb, Ub, Qs, Rs = _random_ltv(rng, 4, 1, 3, 5)
    sat = 0.3

    def run(idx):
        X, U, cost, gains = m4q.quad_program_batch(x0[idx], Xb[idx], Ub[idx], Qs, Rs, A[idx], Bm[idx], D[idx], None, sat, None)
        return dict(X=X, U=U, cost=cost, gains=gains)
    full = run(np.arange(5))
    assert np.abs(full["U"]).max() >= sat * (1 - 1e-15)
    _second_trip(lambda: run(IDX_QUAD), lambda i, place: run(np.array([i])), ("X", "U", "cost", "gains"), kv.QUAD_WRAP, B_QUAD)


def test_plant_step_second_trip():
    c = amc.plant_case(4, 1, kv.HAMILTONIAN)
    rng = np.random.default_rng(9976)
    x5, u5 = c.states(rng, 5), rng.uniform(-c.sat, c.sat, (5, c.m))
    op5, ops5 = c.member_ops(rng, 5)
    _second_trip(lambda: dict(x=m4q.plant_step_batch(x5[IDX_QUAD], u5[IDX_QUAD], op5[IDX_QUAD], ops5[IDX_QUAD], c.dt)),
                 lambda i, place: dict(x=m4q.plant_step_batch(x5[i:i + 1], u5[i:i + 1], op5[i:i + 1], ops5[i:i + 1], c.dt)), ("x",),
                 kv.QUAD_WRAP, B_QUAD)


@pytest.mark.parametrize("kind", [OBSERVE_QUBIT_BLOCK, OBSERVE_PARTIAL_TRACE], ids=["qubit-block-4", "partial-trace-8"])
def test_observe_second_trip(kind):
    n_p, n, _ = observe_dims(kind)
    rng = np.random.default_rng(9977 + kind)
    z5 = rng.standard_normal((5, n_p)) + 1j * rng.standard_normal((5, n_p))
    out = observe_batch(kind, z5)
    assert out.shape == (5, n)
    _second_trip(lambda: dict(x=observe_batch(kind, z5[IDX_QUAD])), lambda i, place: dict(x=observe_batch(kind, z5[i:i + 1])), ("x",),
                 kv.QUAD_WRAP, B_QUAD)

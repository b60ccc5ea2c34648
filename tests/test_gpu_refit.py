"""The DMDc fit against a prior model on the device (dmdc_refit_kernel, dmdc_refit_qr_kernel; m4q_dmdc_refit_batch,
m4q_dmdc_refit_qr_batch): against ONE DiscrepDMDc.fit_iteration of the reference (tests/golden/dmdc_refit.npz), against the NumPy
definitions (fit.dmdc_fit_reference / dmdc_fit_qr_reference with A0, discount, counts), against the plain fit kernels where the
two must agree number for number, across launch layouts, and on the use case: miscalibrated qubits with a short record and a
nominal model.

Bounds, nothing new: the Gram route is held to tests/test_fit_host.py's max(1e-13, 10 eps kappa_r^2) max(1, |A|), the QR route to
tests/test_fit_qr_host.py's max(1e-13 max(1, |A|), 100 sens).  Beside the fixture's cases the shapes are (4,1,1) nz = 8, (4,1,2)
nz = 12, (9,2,1) nz = 27 (two DPP rows in lane_sum), (16,1,2) nz = 48 and (16,3,1) nz = 64 (every lane, the largest LDS layout),
B = 5 and 1, E = 2, N = 24: bilinear members a few per cent apart, each with its neighbour's model as the prior, discount 0.95,
ragged counts.  At nz = 48 and 64 members take fewer snapshots than nz and their data are rank-deficient: every cut-off truncates,
and the QR route may end at its sweep cap (fit.py: the models at the cap are good), so there the status is held to "not 3"."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import fit
from tests.test_fit_host import model_bounds as gram_bounds
from tests.test_fit_qr_host import model_bounds as qr_bounds
from tests.aux_matrix_cases import FIT_B as B, FIT_N as N, synthetic   # (synthetic() lives with the cases of the auxiliary matrix)
from tests.test_refit_host import CASES, FIELDS, load_case, prior_args

pytestmark = pytest.mark.gpu

ROUTES = {"gram": (fit.dmdc_fit_reference, gram_bounds), "qr": (fit.dmdc_fit_qr_reference, qr_bounds)}
SHAPES = [(4, 1, 1), (4, 1, 2), (9, 2, 1), (16, 1, 2), (16, 3, 1)]


def device(c, route, **kw):
    return m4q.dmdc_fit_batch(**dict(prior_args(c), method=route, **kw))


def plain(c, route, **kw):
    args = {k: v for k, v in prior_args(c).items() if k not in ("A0", "discount", "counts")}
    return m4q.dmdc_fit_batch(**dict(args, method=route, **kw))


def same(a, b, members_a=slice(None), members_b=slice(None)):
    """The four results agree as numbers on the chosen members."""
    for f in FIELDS:
        ax = {"models": 1, "rank": 1, "svals": 0, "status": 0}[f]
        x, y = np.moveaxis(a[f], ax, 0)[members_a], np.moveaxis(b[f], ax, 0)[members_b]
        assert np.array_equal(x, y), f


@pytest.fixture(scope="module")
def cases(golden):
    """Every case - the fixture's five and the five synthetic shapes - with what both kernels made of it, computed once."""
    out = {name: load_case(golden, name) for name in CASES}
    out.update({"%d_%d_%d" % s: synthetic(*s) for s in SHAPES})
    return {name: (c, {route: device(c, route) for route in ROUTES}) for name, c in out.items()}


ALL = list(CASES) + ["%d_%d_%d" % s for s in SHAPES]


def check(models, c, bounds, what, name, record_property):
    ratio = float((np.abs(models - c["A"]).max(axis=(2, 3)) / bounds(c)).max())
    record_property("worst_error_over_bound", ratio)
    print("case %s, %s: worst error / bound = %.3g, max error = %.3g" % (name, what, ratio, np.abs(models - c["A"]).max()))
    assert ratio <= 1.0


def status_ok(out, c, route):
    capped = route == "qr" and c["svals"].shape[1] > c["xs"].shape[1] * c["counts"].min()       # rank-deficient by count
    return np.all(out["status"] <= 1) if capped else np.all(out["status"] == 0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ALL)
def test_kernel_matches_the_reference_update(cases, name, route, record_property):
    """The fixture's cases against the reference's fit_iteration, the synthetic ones against NumPy's pinv."""
    c, outs = cases[name]
    out = outs[route]
    assert status_ok(out, c, route), out["status"]
    assert np.array_equal(out["rank"], c["rank"])
    check(out["models"], c, ROUTES[route][1], route + " kernel against the reference", name, record_property)
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    print("case %s, %s: max |s - s_ref| / s_0 per member = %s" % (name, route, err))
    assert np.all(np.diff(out["svals"], axis=1) <= 0) and np.all(err <= 1e-12)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ALL)
def test_kernel_matches_the_definition(cases, name, route, record_property):
    """(Where nz >= 48 the definition, a Python loop over rotations, is evaluated for the first two members only.)"""
    c, outs = cases[name]
    k = 2 if c["A0"].shape[-1] >= 48 else c["xs"].shape[0]
    out = outs[route]
    sub = dict(c, **{f: c[f][:k] for f in ("xs", "A0", "counts", "svals")}, **{f: c[f][:, :k] for f in ("rank", "sens")})
    if c["u_scale"] is not None:
        sub["u_scale"] = c["u_scale"][:k]
    want = ROUTES[route][0](**prior_args(sub))
    assert np.array_equal(out["rank"][:, :k], want["rank"])
    assert status_ok(out, c, route) and status_ok(want, c, route)
    check(out["models"][:, :k], dict(sub, A=want["models"]), ROUTES[route][1], route + " kernel against its definition", name,
          record_property)


# ---------------------------------------------------------------- the identities with the plain fit, number for number
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["%d_%d_%d" % s for s in SHAPES])
def test_identities_with_the_plain_kernel(cases, name, route):
    """A0 = 0, an explicit discount of 1 and full counts each give m4q_dmdc_fit_batch's / m4q_dmdc_fit_qr_batch's numbers, and
    each other's: the discount is a product of its own, a factor 1 changes nothing."""
    c, _ = cases[name]
    want = plain(c, route)
    n, nz = c["A0"].shape[1:]
    full = np.full(B, N, dtype=np.int32)
    for extra in (dict(A0=np.zeros((n, nz))), dict(A0=np.zeros((B, n, nz))), dict(discount=1.0), dict(discount=np.ones(B)),
                  dict(counts=full), dict(A0=np.zeros((B, n, nz)), discount=np.ones(B), counts=full)):
        same(plain(c, route, **extra), want)


# ---------------------------------------------------------------- layouts
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["9_2_1", "16_3_1"])
def test_a_count_equals_cut_trajectories(cases, name, route):
    c, outs = cases[name]
    for b, cnt in enumerate(c["counts"]):
        alone = device(dict(c, xs=c["xs"][b:b + 1, :, :cnt + 1], us=c["us"][:, :cnt], A0=c["A0"][b], counts=None), route)
        same(outs[route], alone, slice(b, b + 1), slice(0, 1))


@pytest.mark.parametrize("route", ROUTES)
def test_members_alone_equal_members_among_261(cases, route):
    c, outs = cases["9_2_1"]
    idx = np.arange(261) % B
    many = device(dict(c, xs=c["xs"][idx], A0=c["A0"][idx], counts=c["counts"][idx]), route)
    for b in range(B):
        alone = device(dict(c, xs=c["xs"][b:b + 1], A0=c["A0"][b:b + 1], counts=c["counts"][b:b + 1]), route)
        same(alone, outs[route], slice(0, 1), slice(b, b + 1))
        for where in (b, 65 + b, 130 + b, 255 + b):
            assert idx[where] == b
            same(alone, many, slice(0, 1), slice(where, where + 1))


@pytest.mark.parametrize("route", ROUTES)
def test_shared_and_per_member_priors_agree(cases, route):
    c, _ = cases["4_1_2"]
    shared = device(dict(c, A0=c["A0"][0], discount=0.95), route)
    per = device(dict(c, A0=np.ascontiguousarray(np.broadcast_to(c["A0"][0], c["A0"].shape)), discount=np.full(B, 0.95)), route)
    same(shared, per)
    mixed = device(dict(c, discount=np.array([0.95, 0.9, 1.0, 0.95, 0.8])), route)
    same(mixed, device(c, route), [0, 3], [0, 3])


@pytest.mark.parametrize("route", ROUTES)
def test_a_member_with_nan_leaves_its_neighbours_alone(cases, route):
    c, outs = cases["9_2_1"]
    xs, A0 = c["xs"].copy(), c["A0"].copy()
    xs[1, 1, 7, 4] = np.nan
    A0[3, 8, 26] = np.nan
    out = device(dict(c, xs=xs, A0=A0), route)
    assert list(out["status"]) == [0, 3, 0, 3, 0]
    assert not out["models"][:, [1, 3]].any() and not out["rank"][:, [1, 3]].any() and not out["svals"][[1, 3]].any()
    same(out, outs[route], [0, 2, 4], [0, 2, 4])


@pytest.mark.parametrize("route", ROUTES)
def test_a_member_without_snapshots_keeps_its_prior(cases, route):
    c, outs = cases["4_1_1"]
    counts = c["counts"].copy()
    counts[2] = 0
    out = device(dict(c, counts=counts), route)
    assert out["status"][2] == 0 and not out["rank"][:, 2].any() and not out["svals"][2].any()
    assert np.array_equal(out["models"][:, 2], np.broadcast_to(c["A0"][2], out["models"][:, 2].shape))
    same(out, outs[route], [0, 1, 3, 4], [0, 1, 3, 4])


# ---------------------------------------------------------------- the use case
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)


def gaussian(amp, centre, width):
    return (amp * np.exp(-0.5 * ((np.arange(N) - centre) / width) ** 2))[:, None]


@pytest.mark.parametrize("route", ROUTES)
def test_miscalibrated_qubits_gain_from_the_prior(route, record_property):
    """Five qubits around the nominal H0 = 0.15 sz, H1 = 0.5 sx (detuning within 20 per cent, drive within 5, as the plant the
    figures of DESIGN 5.5 were taken on), one Gaussian pulse of 24 steps from the ground state as the training record, the
    nominal model discretised at order 2 as the prior.  Validation: prediction_losses on a second pulse from another state.  At a
    truncating cut-off every member's loss after the fit against the prior is below the prior's own and below the plain fit's -
    first for the NumPy definition on the same inputs, then for the kernel."""
    dt, order, rcond = 0.25, 2, 0.045               # rank 5 of 12, a factor 1.2 clear of every member's singular values
    det = 0.15 * (1 + np.array([0.20, -0.10, 0.15, -0.20, 0.10]))
    drv = 0.5 * (1 + np.array([0.05, -0.04, 0.03, 0.05, -0.05]))
    op0, ops = det[:, None, None] * SZ, (drv[:, None, None] * SX)[:, None]
    psi = np.array([np.cos(0.6), np.exp(0.7j) * np.sin(0.6)])
    u_train, u_val = gaussian(1.0, 12.0, 5.0), gaussian(0.8, 9.0, 4.0)
    ground = np.tile(np.array([1, 0, 0, 0], dtype=complex), (B, 1))
    xs_t = m4q.plant_rollout_batch(ground, u_train, op0, ops, dt)["xs"][:, None]
    xs_v = m4q.plant_rollout_batch(np.tile(np.outer(psi, psi.conj()).reshape(-1), (B, 1)), u_val, op0, ops, dt)["xs"][:, None]
    A0 = m4q.discretize_homogeneous_batch([m4q.liouvillian(0.15 * SZ), m4q.liouvillian(0.5 * SX)], dt, order)[0]
    nz = A0.shape[1]

    def losses(models):
        return fit.prediction_losses(xs_v, models[None], u_val[None, None], order)[0]
    prior = losses(np.ascontiguousarray(np.broadcast_to(A0, (B,) + A0.shape)))
    for what, fn in (("definition", ROUTES[route][0]), ("kernel", lambda *a, **k: m4q.dmdc_fit_batch(*a, method=route, **k))):
        against, without = fn(xs_t, u_train, order, rcond, A0=A0), fn(xs_t, u_train, order, rcond)
        assert np.all(against["status"] == 0) and np.all(against["rank"] < nz) and np.array_equal(against["rank"], without["rank"])
        ratio = against["svals"] / (rcond * against["svals"][:, :1])
        assert np.all((ratio >= 1.2) | (ratio <= 1 / 1.2))                      # no rank hangs on rounding
        got, bare = losses(against["models"]), losses(without["models"])
        for b in range(B):
            print("%s, %s, member %d: loss of the prior %.4g, of the plain fit %.4g, of the fit against the prior %.4g"
                  % (route, what, b, prior[b], bare[b], got[b]))
        record_property(what + "_losses", [prior.tolist(), bare.tolist(), got.tolist()])
        assert np.all(got < prior) and np.all(got < bare)


@pytest.mark.parametrize("route", ROUTES)
def test_refit_of_a_run_and_training_against_a_prior(cases, route):
    """refit_models_batch on a stored run against its definition, and train_models_batch(A0=) against a host loop over the device
    fits of its grid."""
    c, _ = cases["4_1_2"]
    run = {"xs": c["xs"][:, 0], "us": np.ascontiguousarray(np.broadcast_to(c["us"][0], (B,) + c["us"][0].shape)), "steps_done": c["counts"]}

    class Clock:
        measure_freq = 1
    got = m4q.refit_models_batch(run, c["A0"], c["order"], Clock(), c["rconds"][-1], discount=0.95, method=route)
    want = m4q.refit_models_batch(run, c["A0"], c["order"], Clock(), c["rconds"][-1], discount=0.95, method=route, reference=True)
    assert np.array_equal(got["rank"], want["rank"]) and np.array_equal(got["status"], want["status"])
    assert np.abs(got["models"] - want["models"]).max() <= 1e-9
    grid = np.array([1e-4, 1e-2, 1e-1])
    trained = m4q.train_models_batch(c["xs"], c["us"], c["order"], rconds=grid, method=route, A0=c["A0"])
    fits = m4q.dmdc_fit_batch(c["xs"], c["us"], c["order"], grid, method=route, A0=c["A0"])
    losses = fit.prediction_losses(c["xs"], fits["models"], c["us"][None], c["order"])
    assert np.array_equal(trained["losses"], losses) and np.array_equal(trained["index"], np.argmin(losses, axis=0))
    assert np.array_equal(trained["models"], fits["models"][trained["index"], np.arange(B)])
    assert not np.array_equal(trained["models"], m4q.train_models_batch(c["xs"], c["us"], c["order"], rconds=grid, method=route)["models"])

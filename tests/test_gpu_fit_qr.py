"""The QR route of the batched DMDc fit on the device (dmdc_fit_qr_kernel, m4q_dmdc_fit_qr_batch) against the reference's
DiscrepDMDc.from_data on ill-conditioned data (tests/golden/dmdc_fit_qr.npz), against its NumPy definition
(fit.dmdc_fit_qr_reference), across launch layouts bit for bit, and through the training workflow.

Bound on a model, against the reference and against the definition alike: |A - A_ref|_inf <= max(1e-13 max(1, |A_ref|_inf), 100 sens)
(tests/test_fit_qr_host.py).  The comparison with the definition is no bit-for-bit claim: the device's sqrt and division and the
compiler's FMA contraction are not NumPy's.  The shapes are the fixture's: nz = 8, 27, 54 and 64 (every lane of the wavefront
busy), two members, or five by repeating them."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import fit
from tests.test_fit_qr_host import CASES, load_case, model_bounds, model_errors, report

pytestmark = pytest.mark.gpu

FIELDS = ("models", "rank", "svals", "status")


def device_fit(c, **kw):
    args = dict(xs=c["xs"], us=c["us"], order=c["order"], rcond=c["rconds"], u_scale=c["u_scale"], method="qr")
    args.update(kw)
    return m4q.dmdc_fit_batch(**args)


@pytest.fixture(scope="module")
def fitted(golden):
    """Every fixture case, what the kernel made of it and what the definition makes of it, computed once and left unchanged."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, device_fit(c), fit.dmdc_fit_qr_reference(c["xs"], c["us"], c["order"], c["rconds"], c["u_scale"]))
    return out


@pytest.fixture(scope="module")
def case_q(fitted):
    return fitted["q"][:2]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_fit(fitted, name, record_property):
    c, out, _ = fitted[name]
    assert np.all(out["status"] == 0), out["status"]
    assert np.array_equal(out["rank"], c["rank"])
    worst = report("kernel error", name, model_errors(out["models"], c), model_bounds(c), record_property)
    assert worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_definition(fitted, name, record_property):
    c, out, want = fitted[name]
    assert np.array_equal(out["rank"], want["rank"]) and np.array_equal(out["status"], want["status"])
    ref = dict(c, A=want["models"])
    worst = report("kernel against definition", name, model_errors(out["models"], ref), model_bounds(ref), record_property)
    assert worst <= 1.0
    for side, sv in (("definition", want["svals"]), ("reference", c["svals"])):
        err = np.abs(out["svals"] - sv).max(axis=1) / c["svals"][:, 0]
        record_property("sval_error_over_s0_against_" + side, float(err.max()))
        print("case %s: max |s - s_%s| / s_0 per member = %s" % (name, side, err))
        assert np.all(err <= 1e-12)
    assert np.all(np.diff(out["svals"], axis=1) <= 0)


# ---------------------------------------------------------------- layout invariances, bit for bit
@pytest.mark.parametrize("name", ["q", "s"])
def test_member_alone_equals_member_in_a_ragged_launch(fitted, name):
    """Each member alone (B = 1) and among five (the two repeated)."""
    c = fitted[name][0]
    idx = np.array([0, 1, 1, 0, 1])
    many = device_fit(c, xs=c["xs"][idx], u_scale=c["u_scale"][idx])
    for b in range(2):
        one = device_fit(c, xs=c["xs"][b:b + 1], u_scale=c["u_scale"][b:b + 1])
        for where in np.nonzero(idx == b)[0]:
            assert np.array_equal(one["models"][:, 0], many["models"][:, where])
            assert np.array_equal(one["rank"][:, 0], many["rank"][:, where])
            assert np.array_equal(one["svals"][0], many["svals"][where]) and one["status"][0] == many["status"][where]


def test_shared_controls_equal_repeated_controls(case_q):
    c, out = case_q
    assert c["us"].ndim == 3
    per = device_fit(c, us=np.ascontiguousarray(np.broadcast_to(c["us"], (2,) + c["us"].shape)))
    for f in FIELDS:
        assert np.array_equal(per[f], out[f]), f


def test_one_cutoff_at_a_time_equals_all_at_once(case_q):
    c, out = case_q
    assert len(np.unique(out["rank"])) >= 2
    for r, rc in enumerate(c["rconds"]):
        one = device_fit(c, rcond=float(rc))
        assert np.array_equal(one["models"], out["models"][r]) and np.array_equal(one["rank"], out["rank"][r])
        assert np.array_equal(one["svals"], out["svals"]) and np.array_equal(one["status"], out["status"])


def test_one_experiment_equals_the_same_snapshots_cut_in_two(case_q):
    """E = 1, N = 40 against E = 2, N = 20: the second experiment starts at the state the first one ends in."""
    c, out = case_q
    xs, us = c["xs"], c["us"]
    assert xs.shape[1] == 1 and us.shape[:2] == (1, 40)
    xs2 = np.ascontiguousarray(np.stack([xs[:, 0, :21], xs[:, 0, 20:]], axis=1))
    us2 = np.ascontiguousarray(us[0].reshape(2, 20, -1))
    cut = device_fit(c, xs=xs2, us=us2)
    for f in FIELDS:
        assert np.array_equal(cut[f], out[f]), f


# ---------------------------------------------------------------- non-finite data
def test_a_member_with_nan_leaves_its_neighbours_alone(case_q):
    c, _ = case_q
    idx = np.array([0, 1, 0, 1, 0])
    base = device_fit(c, xs=c["xs"][idx], u_scale=c["u_scale"][idx])
    xs = c["xs"][idx].copy()
    xs[2, 0, 17, 4] = np.nan
    out = device_fit(c, xs=xs, u_scale=c["u_scale"][idx])
    assert list(out["status"]) == [0, 0, 3, 0, 0]
    assert not out["models"][:, 2].any() and not out["rank"][:, 2].any() and not out["svals"][2].any()
    keep = [0, 1, 3, 4]
    assert np.array_equal(out["models"][:, keep], base["models"][:, keep])
    assert np.array_equal(out["rank"][:, keep], base["rank"][:, keep]) and np.array_equal(out["svals"][keep], base["svals"][keep])
    xs = c["xs"][idx].copy()
    xs[4, 0, 40, 0] = np.inf                                                       # in the last x_{t+1} alone
    assert list(device_fit(c, xs=xs, u_scale=c["u_scale"][idx])["status"]) == [0, 0, 0, 0, 3]


# ---------------------------------------------------------------- the training workflow
def test_training_picks_the_host_loops_cutoff(case_q):
    """train_models_batch(method="qr") on case q over the fixture's cut-offs (1e-10 among them) against the reference's workflow
    member by member: DiscrepDMDc.from_data per cut-off, each candidate rolled by model_rollout_batch, the first smallest loss
    kept."""
    c, _ = case_q
    xs, us, u_scale, order, grid = c["xs"], c["us"], c["u_scale"], c["order"], c["rconds"]
    B, E, _, n = xs.shape
    got = m4q.train_models_batch(xs, us, order, rconds=grid, u_scale=u_scale, method="qr")
    assert np.all(got["status"] == 0) and got["losses"].shape == (len(grid), B)
    for b in range(B):
        Z, Y = fit.stack_snapshots(xs[b], u_scale[b] * us, order)
        best, best_r = np.inf, None
        for r, rc in enumerate(grid):
            A = m4q.DiscrepDMDc.from_data(Y, Z[:n], Z[n:], rcond=rc).A
            loss = 0.0
            for e in range(E):
                pred = m4q.model_rollout_batch(xs[b:b + 1, e, 0], u_scale[b] * us[e], A, order, keep="all")["xs"][0]
                loss += np.linalg.norm((xs[b, e, 1:] - pred[1:]).T, 2)
            if loss < best:
                best, best_r = loss, r
        print("member %d: device losses %s, host loop's best %.3g at %d" % (b, got["losses"][:, b], best, best_r))
        assert got["index"][b] == best_r and got["rcond"][b] == grid[best_r], (b, got["losses"][:, b], best)

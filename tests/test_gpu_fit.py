"""The batched DMDc fit on the device (dmdc_fit_kernel, m4q_dmdc_fit_batch) against the reference's DiscrepDMDc.from_data
(tests/golden/dmdc_fit.npz), against its NumPy definition (fit.dmdc_fit_reference), across launch layouts bit for bit, and round
the loop rollout -> fit without any reference.

Bound on a model, everywhere: |A - A_ref| <= max(1e-13, 10 eps kappa^2) max(1, |A_ref|_inf) with kappa = s_0 / s_r of the data (r the
rank kept) - the forward error of a normal-equations solve (tests/test_fit_host.py).  The comparison with the definition is held to
the same bound and its measured figure recorded: it is not a bit-for-bit claim, the device's sqrt and division and the compiler's
FMA contraction are not NumPy's.  The shapes are the fixture's: nz = 8, 12, 24, 27 and 64 (every lane of the wavefront busy),
B = 1 to 67 (a grid of its own per member)."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import configs, fit
from mpc4quantum_amd.mpc import open_session
from tests.test_fit_host import CASES, EPS, load_case, worst_over_bound

pytestmark = pytest.mark.gpu


def device_fit(c, **kw):
    args = dict(xs=c["xs"], us=c["us"], order=c["order"], rcond=c["rconds"], u_scale=c["u_scale"])
    args.update(kw)
    return m4q.dmdc_fit_batch(**args)


@pytest.fixture(scope="module")
def fitted(golden):
    """Every fixture case and what the kernel made of it, computed once and left unchanged."""
    out = {}
    for name in CASES:
        c = load_case(golden, name)
        out[name] = (c, device_fit(c))
    return out


@pytest.fixture(scope="module")
def case_b(fitted):
    return fitted["b"]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_fit(fitted, name, record_property):
    c, out = fitted[name]
    assert np.all(out["status"] == 0), out["status"]
    assert np.array_equal(out["rank"], c["rank"])
    worst = worst_over_bound(out["models"], c)
    record_property("worst_error_over_bound", worst)
    print("case %s: worst |A - A_ref| / bound = %.3g, max |A - A_ref| = %.3g" % (name, worst, np.abs(out["models"] - c["A"]).max()))
    assert worst <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_kernel_singular_values(fitted, name, record_property):
    """svals to 1e-12 s_0, the two null singular values of case a (rank 6 of 8, 1e-17 s_0 in the fixture) included: svals is
    sqrt(sum |v_k^H z|^2) over the snapshots, not sqrt(lam_k), which would sit at G's rounding floor there (sqrt(nz eps) s_0 ~
    4e-8 s_0).  The definition in NumPy gives 2e-16 to 7e-15 s_0 over the five cases; the device figure is printed below."""
    c, out = fitted[name]
    err = np.abs(out["svals"] - c["svals"]).max(axis=1) / c["svals"][:, 0]
    record_property("worst_sval_error_over_s0", float(err.max()))
    print("case %s: max |s - s_ref| / s_0 per member = %s" % (name, err))
    assert np.all(np.diff(out["svals"], axis=1) <= 0)
    assert np.all(err <= 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_definition(fitted, name, record_property):
    c, out = fitted[name]
    want = fit.dmdc_fit_reference(c["xs"], c["us"], c["order"], c["rconds"], c["u_scale"])
    assert np.array_equal(out["rank"], want["rank"]) and np.array_equal(out["status"], want["status"])
    worst = worst_over_bound(out["models"], dict(c, A=want["models"]))
    measured = float(np.abs(out["models"] - want["models"]).max())
    record_property("max_error_against_definition", measured)
    record_property("worst_error_over_bound", worst)
    print("case %s: max |A_device - A_definition| = %.3g, over the bound %.3g" % (name, measured, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- layout invariances, bit for bit
FIELDS = ("models", "rank", "svals", "status")


def test_member_alone_equals_member_in_a_ragged_grid(case_b):
    """Each member of case b alone (B = 1) and among 67 members (the five repeated)."""
    c, _ = case_b
    idx = np.arange(67) % 5
    many = device_fit(c, xs=c["xs"][idx], u_scale=c["u_scale"][idx])
    for b in range(5):
        one = device_fit(c, xs=c["xs"][b:b + 1], u_scale=c["u_scale"][b:b + 1])
        for where in (b, 65 + b if b < 2 else 60 + b):
            assert np.array_equal(one["models"][:, 0], many["models"][:, where])
            assert np.array_equal(one["rank"][:, 0], many["rank"][:, where])
            assert np.array_equal(one["svals"][0], many["svals"][where]) and one["status"][0] == many["status"][where]


def test_shared_controls_equal_repeated_controls(case_b):
    c, out = case_b
    assert c["us"].ndim == 3
    per = device_fit(c, us=np.ascontiguousarray(np.broadcast_to(c["us"], (5,) + c["us"].shape)))
    for f in FIELDS:
        assert np.array_equal(per[f], out[f]), f


def test_u_scale_equals_controls_scaled_on_the_host(case_b):
    c, out = case_b
    scaled = c["u_scale"][:, None, None, :] * c["us"][None]                 # the same fp64 product
    pre = device_fit(c, us=scaled, u_scale=None)
    for f in FIELDS:
        assert np.array_equal(pre[f], out[f]), f


def test_one_cutoff_at_a_time_equals_all_at_once(case_b):
    c, _ = case_b
    rconds = c["rconds"][[0, 2, 3]]
    all3 = device_fit(c, rcond=rconds)
    assert len(np.unique(all3["rank"])) >= 2
    for r, rc in enumerate(rconds):
        one = device_fit(c, rcond=float(rc))
        assert np.array_equal(one["models"], all3["models"][r]) and np.array_equal(one["rank"], all3["rank"][r])
        assert np.array_equal(one["svals"], all3["svals"]) and np.array_equal(one["status"], all3["status"])


# ---------------------------------------------------------------- round trip without a reference
@pytest.mark.parametrize("n,m,order,B,E,N", [(4, 2, 1, 5, 3, 9), (9, 2, 2, 3, 5, 23), (16, 1, 2, 2, 6, 17), (16, 1, 3, 2, 8, 17)],
                         ids=lambda v: str(v))
def test_models_survive_rollout_and_fit(n, m, order, B, E, N, record_property):
    """Random stable models under full-rank excitation, through model_rollout_batch and back through dmdc_fit_batch."""
    rng = np.random.default_rng(100 * n + 10 * m + order)
    P = m4q.size_of_library(order, m) - 1
    nz = n * (1 + P)
    models = np.zeros((B, n, nz), dtype=complex)
    for b in range(B):
        A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        models[b, :, :n] = A * (0.9 / np.abs(np.linalg.eigvals(A)).max())
        models[b, :, n:] = 0.3 * (rng.standard_normal((n, n * P)) + 1j * rng.standard_normal((n, n * P))) / np.sqrt(n * P)
    us = rng.uniform(-1, 1, (B, E, N, m))
    x0 = rng.standard_normal((B, E, n)) + 1j * rng.standard_normal((B, E, n))
    xs = np.stack([m4q.model_rollout_batch(x0[:, e], us[:, e], models, order, keep="all")["xs"] for e in range(E)], axis=1)
    out = m4q.dmdc_fit_batch(xs, us, order, 1e-6)
    assert np.all(out["status"] == 0) and np.all(out["rank"] == nz)
    worst = 0.0
    for b in range(B):
        s = np.linalg.svd(fit.stack_snapshots(xs[b], us[b], order)[0], compute_uv=False)
        assert s[-1] > 1.2e-6 * s[0]                                        # full rank at this cut-off, with the fixture's margin
        kappa = s[0] / s[-1]
        bound = max(1e-13, 10 * EPS * kappa ** 2) * max(1.0, np.abs(models[b]).max())
        worst = max(worst, np.abs(out["models"][b] - models[b]).max() / bound)
        # (a Gram eigenvalue moves by nz eps lam_max at the most, so s_i by nz eps kappa s_0 / 2 < 1e-14 kappa s_0)
        assert np.abs(out["svals"][b] - s).max() <= 1e-14 * s[0] * max(1.0, kappa)
    record_property("worst_error_over_bound", worst)
    print("(%d, %d, %d): worst |A_fit - A| / bound = %.3g" % (n, m, order, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- non-finite data
def test_a_member_with_nan_leaves_its_neighbours_alone(case_b):
    c, clean = case_b
    xs = c["xs"].copy()
    xs[2, 1, 17, 4] = np.nan
    out = device_fit(c, xs=xs)
    assert list(out["status"]) == [0, 0, 3, 0, 0]
    assert not out["models"][:, 2].any() and not out["rank"][:, 2].any() and not out["svals"][2].any()
    keep = [0, 1, 3, 4]
    assert np.array_equal(out["models"][:, keep], clean["models"][:, keep])
    assert np.array_equal(out["rank"][:, keep], clean["rank"][:, keep]) and np.array_equal(out["svals"][keep], clean["svals"][keep])
    us = np.ascontiguousarray(np.broadcast_to(c["us"], (5,) + c["us"].shape)).copy()
    us[4, 0, 3, 1] = np.inf
    assert list(device_fit(c, us=us)["status"]) == [0, 0, 0, 0, 3]


# ---------------------------------------------------------------- the training workflow
def test_training_picks_the_host_loops_model_and_a_session_takes_it(case_b):
    """train_models_batch on case b against the reference's workflow member by member: DiscrepDMDc.from_data over the grid of
    rcond, each candidate rolled by model_rollout_batch, the first smallest loss kept.  The chosen models then drive a closed
    loop: a session takes fitted models as it takes discretised ones."""
    c, _ = case_b
    xs, us, u_scale, order = c["xs"], c["us"], c["u_scale"], c["order"]
    B, E = xs.shape[:2]
    grid = np.logspace(-6, -1, 10)
    got = m4q.train_models_batch(xs, us, order, u_scale=u_scale)
    assert np.all(got["status"] == 0) and got["losses"].shape == (10, B)
    for b in range(B):
        Z, Y = fit.stack_snapshots(xs[b], u_scale[b] * us, order)
        n = xs.shape[-1]
        best, best_r = np.inf, None
        for r, rc in enumerate(grid):
            A = m4q.DiscrepDMDc.from_data(Y, Z[:n], Z[n:], rcond=rc).A
            loss = 0.0
            for e in range(E):
                pred = m4q.model_rollout_batch(xs[b:b + 1, e, 0], u_scale[b] * us[e], A, order, keep="all")["xs"][0]
                loss += np.linalg.norm((xs[b, e, 1:] - pred[1:]).T, 2)
            if loss < best:
                best, best_r = loss, r
        assert got["index"][b] == best_r and got["rcond"][b] == grid[best_r], (b, got["losses"][:, b], best)
    p = configs.build(3, batch=B, horizon=8, n_steps=3, drift_scale=0.125)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    sess = open_session(p["x0"], got["models"], p["dim_u"], order, p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"],
                        p["Q"], p["R"], p["Qf"], p["sat"], p["du"])
    try:
        sess.run(0, 3)
        res = sess.results()
        assert np.all(res["exit_codes"] == 0) and np.all(res["steps_done"] == 3), (res["exit_codes"], res["steps_done"])
    finally:
        sess.close()

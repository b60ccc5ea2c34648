"""The batched recursive DMDc update on the device (online_dmdc_kernel, m4q_online_dmdc_batch) against its NumPy definition
(online.online_dmdc_reference), against what the reference's OnlineDMDc recorded (tests/golden/online_dmdc.npz), across launch
layouts bit for bit, and round the loop: mpc_batch, then stream_models_batch, against the drop-in mpc(..., streaming=True).

Bound, everywhere a device result meets a NumPy one: max(1e-12, 100 s) relative to each member's max |A| / max |P| (max innovation
for the innovations), where s is how far the definition itself moves when the data are perturbed by a relative 1e-15 - measured
here per case, and asserted to stay under 1e-11 first, so the bound never exceeds 1e-9.  The recursion is not contractive: its
rounding error grows with 1 / discount^N and, in the plain (unconjugated) form, with 1 / |1 + z^T P z|, which nothing keeps away
from zero; discounts below 0.95 and N in the hundreds are deliberately not test inputs (at discount = 0.9, N = 200 the
reference's own recursion moves by 3e-3).  The cases are tests/test_online_host.py's: nz = 8, 27, 64 (every lane busy) and 32."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs, online
from tests.test_online_host import ALPHA, CASES, call_args, load_case, rel_err, two_experiments

pytestmark = pytest.mark.gpu
FIELDS = ("models", "P", "hist", "innov", "status")


def jitter(a, rng):
    return a * (1 + 1e-15 * rng.standard_normal(a.shape))


def sensitivity(args, want, draws=3):
    """(s_A, s_P, s_innov): the largest relative move of the definition's outputs over `draws` perturbations of xs and us by a
    relative 1e-15 (one draw sees one direction; the largest of three is still an underestimate of the worst)."""
    rng = np.random.default_rng(31)
    s = np.zeros(3)
    for _ in range(draws):
        moved = online.online_dmdc_reference(**dict(args, xs=jitter(args["xs"], rng), us=jitter(args["us"], rng)))
        s = np.maximum(s, [rel_err(moved["models"], want["models"]), rel_err(moved["P"], want["P"]),
                           float((np.abs(moved["innov"] - want["innov"]).max(axis=1) / want["innov"].max(axis=1)).max())])
    return s


@pytest.fixture(scope="module")
def computed(golden):
    """(case, E, hermitian) -> (inputs, the kernel's result, the definition's, s): computed once and left unchanged."""
    out = {}
    for name in CASES:
        one = load_case(golden, name)
        for E, c in ((1, one), (2, two_experiments(one))):
            for hermitian in (False, True):
                args = call_args(c, hermitian=hermitian, hist_every=5, innovations=True)
                want = online.online_dmdc_reference(**args)
                out[name, E, hermitian] = (c, m4q.online_dmdc_batch(**args), want, sensitivity(args, want))
    return out


def against(got, want, s, record_property, what):
    """The module docstring's bound on models, P, hist and innov; every measured figure printed and recorded first."""
    assert np.all(s <= 1e-11), s
    bA, bP, bI = (max(1e-12, 100 * v) for v in s)
    eA, eP = rel_err(got["models"], want["models"]), rel_err(got["P"], want["P"])
    eH = rel_err(got["hist"], want["hist"], np.broadcast_to(want["models"], want["hist"].shape)) if want["hist"].size else 0.0
    eI = float((np.abs(got["innov"] - want["innov"]).max(axis=1) / want["innov"].max(axis=1)).max())
    for k, v in (("s_A", s[0]), ("s_P", s[1]), ("s_innov", s[2]), ("err_A", eA), ("err_P", eP), ("err_hist", eH), ("err_innov", eI)):
        record_property(k, float(v))
    print("%s: s = %.3g / %.3g / %.3g (A / P / innov); errors A %.3g, P %.3g, hist %.3g, innov %.3g"
          % (what, s[0], s[1], s[2], eA, eP, eH, eI))
    assert np.array_equal(got["status"], want["status"]) and np.all(got["status"] == 0)
    assert got["hist"].shape == want["hist"].shape and got["innov"].shape == want["innov"].shape
    assert eA <= bA and eH <= bA and eP <= bP and eI <= bI


@pytest.mark.parametrize("hermitian", [False, True], ids=["plain", "hermitian"])
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_definition(computed, name, E, hermitian, record_property):
    _, got, want, s = computed[name, E, hermitian]
    against(got, want, s, record_property, "case %s E=%d %s" % (name, E, "hermitian" if hermitian else "plain"))


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_class(computed, name, record_property):
    """The A and P the reference's own OnlineDMDc held after the last update, and its A after updates 5, 10, ..."""
    c, got, _, s = computed[name, 1, False]
    assert np.all(s <= 1e-11), s
    eA, eP = rel_err(got["models"], c["A"]), rel_err(got["P"], c["P"])
    eH = rel_err(got["hist"], c["A_hist"], np.broadcast_to(c["A"], c["A_hist"].shape))
    record_property("err_A", eA)
    record_property("err_P", eP)
    print("case %s against the reference's class: A %.3g, P %.3g, hist %.3g" % (name, eA, eP, eH))
    assert eA <= max(1e-12, 100 * s[0]) and eH <= max(1e-12, 100 * s[0]) and eP <= max(1e-12, 100 * s[1])


@pytest.mark.parametrize("name", CASES)
def test_two_experiments_are_the_same_snapshots(computed, name):
    """The trajectory cut in two is the same sequence of updates: bit for bit, both forms."""
    for hermitian in (False, True):
        for f in FIELDS:
            assert np.array_equal(computed[name, 1, hermitian][1][f], computed[name, 2, hermitian][1][f]), f


# ---------------------------------------------------------------- layout invariances, bit for bit
@pytest.fixture(scope="module")
def five(golden):
    """Five different members from case c's two: their own A0 and discount."""
    c = load_case(golden, "c")
    idx = np.array([0, 1, 0, 1, 0])
    return dict(xs=np.ascontiguousarray(c["xs"][idx]), us=c["us"], order=1, u_scale=np.ascontiguousarray(c["u_scale"][idx]),
                A0=np.stack([c["A0"] * (1 + 0.01 * b) for b in range(5)]), alpha=ALPHA, discount=np.array([0.97, 0.97, 0.95, 0.96, 1.0]),
                hist_every=5, innovations=True)


def take(args, idx):
    return dict(args, xs=np.ascontiguousarray(args["xs"][idx]), u_scale=np.ascontiguousarray(args["u_scale"][idx]),
                A0=np.ascontiguousarray(args["A0"][idx]), discount=np.ascontiguousarray(args["discount"][idx]))


def test_member_alone_equals_member_in_a_grid_stride_loop(five):
    """Each of five members alone (B = 1) and at four places among 4,099: more members than workgroups, members 4096 to 4098 are
    a workgroup's second."""
    many = m4q.online_dmdc_batch(**take(five, np.arange(4099) % 5))
    assert np.all(many["status"] == 0)
    for b in range(5):
        one = m4q.online_dmdc_batch(**take(five, [b]))
        for where in (b, 2000 + b, 4090 + b, 4095 + b if b in (1, 2, 3) else 4085 + b):
            assert where % 5 == b
            assert np.array_equal(one["models"][0], many["models"][where]) and np.array_equal(one["P"][0], many["P"][where])
            assert np.array_equal(one["hist"][:, 0], many["hist"][:, where]) and np.array_equal(one["innov"][0], many["innov"][where])


def test_shared_arguments_equal_repeated_ones(computed):
    c, out, _, _ = computed["b", 2, True]
    B, nz = c["xs"].shape[0], 8
    per = m4q.online_dmdc_batch(c["xs"], np.ascontiguousarray(np.broadcast_to(c["us"], (B,) + c["us"].shape)), 1,
                                np.ascontiguousarray(np.broadcast_to(c["A0"], (B,) + c["A0"].shape)),
                                P0=np.ascontiguousarray(np.broadcast_to(ALPHA * np.identity(nz), (B, nz, nz))),
                                discount=np.full(B, c["discount"]), u_scale=c["u_scale"], hermitian=True, hist_every=5, innovations=True)
    for f in FIELDS:
        assert np.array_equal(per[f], out[f]), f


def test_alpha_equals_an_explicit_p0_and_hist_changes_nothing_else(computed):
    c, out, _, _ = computed["e", 1, False]
    args = call_args(c, hist_every=5, innovations=True)
    explicit = m4q.online_dmdc_batch(**dict(args, alpha=None, P0=ALPHA * np.identity(32)))
    for f in FIELDS:
        assert np.array_equal(explicit[f], out[f]), f
    plain = m4q.online_dmdc_batch(**call_args(c))
    assert plain["hist"].shape == (0, 2, 16, 32) and "innov" not in plain
    assert np.array_equal(plain["models"], out["models"]) and np.array_equal(plain["P"], out["P"])
    assert np.array_equal(plain["status"], out["status"])


def test_ragged_counts_equal_runs_on_truncated_data(golden):
    c = two_experiments(load_case(golden, "c"))                         # [2, 2, 21, 9]
    idx = np.array([0, 1, 0, 1, 1])
    counts = np.array([20, 7, 0, 13, 1])
    args = call_args(c, xs=np.ascontiguousarray(c["xs"][idx]), u_scale=np.ascontiguousarray(c["u_scale"][idx]), hist_every=5,
                     innovations=True, hermitian=True)
    out = m4q.online_dmdc_batch(**dict(args, counts=counts))
    assert np.all(out["status"] == 0) and out["hist"].shape[0] == 8 and out["innov"].shape == (5, 40)
    for b, cnt in enumerate(counts):
        if cnt == 0:
            assert np.array_equal(out["models"][b], c["A0"]) and np.array_equal(out["P"][b], ALPHA * np.identity(27))
            assert not out["hist"][:, b].any() and not out["innov"][b].any()
            continue
        cut = m4q.online_dmdc_batch(**dict(args, xs=np.ascontiguousarray(args["xs"][b:b + 1, :, :cnt + 1]),
                                           us=np.ascontiguousarray(c["us"][:, :cnt]), u_scale=args["u_scale"][b:b + 1]))
        H = (2 * cnt) // 5
        assert cut["hist"].shape[0] == H
        assert np.array_equal(out["models"][b], cut["models"][0]) and np.array_equal(out["P"][b], cut["P"][0])
        assert np.array_equal(out["hist"][:H, b], cut["hist"][:, 0]) and not out["hist"][H:, b].any()
        inn = out["innov"][b].reshape(2, 20)
        assert np.array_equal(inn[:, :cnt], cut["innov"][0].reshape(2, cnt)) and not inn[:, cnt:].any()


def test_a_member_with_nan_leaves_its_neighbours_alone(computed):
    c, clean, _, _ = computed["a", 1, False]
    idx = [0, 1, 0, 1]
    args = call_args(c, xs=np.ascontiguousarray(c["xs"][idx]), u_scale=np.ascontiguousarray(c["u_scale"][idx]), hist_every=5,
                     innovations=True)
    args["xs"][2, 0, 6, 2] = np.nan
    out = m4q.online_dmdc_batch(**args)
    assert list(out["status"]) == [0, 0, 3, 0]
    assert not out["models"][2].any() and not out["P"][2].any() and not out["hist"][:, 2].any()
    for b in (0, 1, 3):
        for f in ("models", "P", "innov"):
            assert np.array_equal(out[f][b], clean[f][idx[b]]), (f, b)
        assert np.array_equal(out["hist"][:, b], clean["hist"][:, idx[b]])
    us = np.ascontiguousarray(np.broadcast_to(c["us"], (4, 1) + c["us"].shape)).copy()
    us[1, 0, 3, 0] = np.inf
    assert list(m4q.online_dmdc_batch(**dict(args, xs=np.ascontiguousarray(c["xs"][idx]), us=us))["status"]) == [0, 3, 0, 0]


def test_unsupported_shape():
    with pytest.raises(_lib.M4qError) as err:
        m4q.online_dmdc_batch(np.zeros((2, 5, 16)), np.zeros((4, 1)), 4, np.zeros((16, 80)), alpha=ALPHA)
    assert err.value.code == _lib.E_UNSUPPORTED


# ---------------------------------------------------------------- round the loop
def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("config", [1, 3])
def test_streaming_for_an_ensemble_equals_the_drop_in(config, record_property):
    """mpc_batch, then stream_models_batch, against mpc(..., streaming=True) around OnlineDMDc.from_bootstrap(alpha=1e2), member by
    member, at T = 10 and measure_freq = 1: the model handed back within the bound of the module docstring (s measured on the
    run), the runs themselves as test_mpc_streaming_refits_the_model_object asks of a run the refit does not steer (1e-8)."""
    B, ns = 3, 10
    p = configs.build(config, batch=B, horizon=10, n_steps=ns)
    n, m = p["dim_x"], p["dim_u"]
    models = np.ascontiguousarray(np.broadcast_to(p["models"], (B,) + p["models"].shape[1:]))
    op0 = np.stack([(1 + 0.05 * b) * p["plant_op0"][0] for b in range(B)])          # three different plants
    ops = np.ascontiguousarray(np.broadcast_to(p["plant_ops"], (B,) + p["plant_ops"].shape[1:]))
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    run = m4q.mpc_batch(p["x0"], models, m, p["order"], p["X_targ"], p["U_targ"], clock, op0, ops, p["Q"], p["R"], p["Qf"], p["sat"],
                        p["du"])
    assert np.all(run["exit_codes"] == 0) and np.all(run["steps_done"] == ns)
    got = m4q.stream_models_batch(run, models, p["order"], clock, alpha=ALPHA, innovations=True)
    assert np.all(got["status"] == 0)
    xs = np.ascontiguousarray(np.swapaxes(run["xs"], 1, 2))
    us = np.ascontiguousarray(np.swapaxes(run["us"], 1, 2))
    args = dict(xs=xs, us=us, order=p["order"], A0=models, alpha=ALPHA, innovations=True)
    s = sensitivity(args, online.online_dmdc_reference(**args))
    assert np.all(s <= 1e-11), s
    worst = np.zeros(4)
    for b in range(B):
        model = m4q.OnlineDMDc.from_bootstrap(n, n, models.shape[2] - n, models[b].copy(), alpha=ALPHA)
        (xd, ud), back, code = m4q.mpc(p["x0"][b], m, p["order"], p["X_targ"], p["U_targ"], m4q.StepClock(p["dt"], p["horizon"], ns),
                                       m4q.QExperiment(op0[b], list(ops[b])), model, p["Q"], p["R"], p["Qf"], sat=p["sat"],
                                       du=p["du"], streaming=True, progress_bar=False)
        assert code == 0 and back is model and model._iteration == ns
        worst = np.maximum(worst, [rel_err(got["models"][b], model.A), rel_err(got["P"][b], model.P), rel(run["xs"][b], xd),
                                   rel(run["us"][b], ud)])
        again = m4q.OnlineDMDc.from_batch(got, b)
        assert np.array_equal(again.A, got["models"][b]) and np.array_equal(again.P, got["P"][b])
    for k, v in zip(("s_A", "s_P", "err_A", "err_P", "err_xs", "err_us"), list(s[:2]) + list(worst)):
        record_property(k, float(v))
    print("config %d: s = %.3g / %.3g; model A %.3g, P %.3g; runs xs %.3g, us %.3g" % (config, s[0], s[1], *worst))
    assert worst[2] <= 1e-8 and worst[3] <= 1e-8
    assert worst[0] <= max(1e-12, 100 * s[0]) and worst[1] <= max(1e-12, 100 * s[1])
    assert np.abs(got["models"] - models).max() > 1e-6                                # refitted

"""The robust optimiser on the device (m4q_plant_robust_batch) and the kernel its line search runs on (plant_rollout_multi_kernel,
m4q_plant_rollout_multi_batch): the multi rollout against plant_rollout_batch and ordered_weighted_sum bit for bit at every built
shape and kind; the one call against the definition driven by the package's earlier device entry points, bit for bit; against the
pure NumPy definition with a bound measured on the definition itself; chaining; the statuses; descent on config 1's ensemble.

Shapes are the smallest that can go wrong: B = 7 and 11 (ragged quads), N = 5 and 6; B = 259 for the reduction (two chunks, the
second ragged); one case with 4,098 quads, past the grid the launch is capped at."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import configs
from mpc4quantum_amd import plant_robust as pr
from tests import plant_robust_cases as rc

pytestmark = pytest.mark.gpu

HAMILTONIAN = ("4-1", "4-2", "9-2", "16-1", "16-2", "16-3")          # every built (n, m), the plant-only (16, 2) included
PROCESS = ("16-1-process", "16-2-process", "16-3-process")
ALL = HAMILTONIAN + PROCESS


# ---------------------------------------------------------------- 1. the multi kernel
def _multi_check(name, B, N, S, figure, weighted, seed):
    k = rc.case(name, B, N, seed)
    x0, U0, op0, ops, ts, W, f, sat = k["args"]
    rng = np.random.default_rng(seed + 1)
    us = rng.uniform(-sat, sat, (S, N, U0.shape[1]))
    us[0] = U0
    kw = dict(k["kw"], figure=figure)
    if not weighted:
        kw["weights"] = None
    out = m4q.plant_rollout_multi_batch(x0, us, op0, ops, ts, W, f, **kw)
    assert out["J"].shape == (B, S) and out["F"].shape == (S,) and np.isfinite(out["J"]).all()
    for s in range(S):
        assert np.array_equal(out["J"][:, s], rc.member_objectives(k, us[s], figure)), (name, s)
    assert np.array_equal(out["F"], m4q.ordered_weighted_sum(out["J"], kw["weights"]))
    again = m4q.plant_rollout_multi_batch(x0, us, op0, ops, ts, W, f, **kw)
    assert np.array_equal(again["J"], out["J"]) and np.array_equal(again["F"], out["F"])
    # each output alone is the same output
    only_F = m4q.plant_rollout_multi_batch(x0, us, op0, ops, ts, W, f, members=False, **kw)
    only_J = m4q.plant_rollout_multi_batch(x0, us, op0, ops, ts, W, f, mean=False, **kw)
    assert set(only_F) == {"F"} and set(only_J) == {"J"}
    assert np.array_equal(only_F["F"], out["F"]) and np.array_equal(only_J["J"], out["J"])
    assert np.ptp(out["J"], axis=0).min() > 0 and (S == 1 or np.ptp(out["F"]) > 0)          # (members and sequences differ)


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "uniform"])
@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("name", ALL)
def test_multi_rollout_equals_the_rollout_and_the_ordered_sum(name, figure, weighted):
    _multi_check(name, 7, 5, 3, figure, weighted, 9600 + 7 * ALL.index(name))


@pytest.mark.parametrize("B,N,S", [(7, 5, 1), (7, 5, 8), (259, 5, 3), (16389, 2, 2)], ids=str)
def test_multi_rollout_at_the_edges_of_s_the_chunks_and_the_grid(B, N, S):
    _multi_check("4-1", B, N, S, "sum", True, 9700 + S)


# ---------------------------------------------------------------- 2. the one call against the definition driven by the device
LOOP = dict(iters=4, steps=4, step0=rc.STEP0, tol=0.0)
HISTORY = ("U", "cost_hist", "alpha_hist", "pgrad_hist")


def _same_run(got, want):
    for key in HISTORY:
        assert np.array_equal(got[key], want[key]), key
    assert (got["cost"], got["n_iter"], got["status"]) == (want["cost"], want["n_iter"], want["status"])


@pytest.mark.parametrize("mem", [0, 3])
@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_one_call_equals_the_definition_on_the_device_entry_points(name, figure, mem):
    k = rc.case(name, 11, 6, 9800 + 5 * rc.NAMES.index(name))
    trace = []
    want = m4q.plant_robust_reference(*k["args"], figure=figure, mem=mem, evaluate=rc.device_evaluate(k, figure), trace=trace, **k["kw"],
                                      **LOOP)
    got = m4q.plant_robust_batch(*k["args"], figure=figure, mem=mem, members=True, **k["kw"], **LOOP)
    _same_run(got, want)
    assert np.count_nonzero(got["alpha_hist"]) >= 2 and got["cost"] < got["cost_hist"][0]
    if mem:
        print("%s %s: pairs in use per iteration %s" % (name, figure, [t["used"] for t in trace]))
    x0, _, op0, ops, ts, W, f, _ = k["args"]
    at = m4q.plant_rollout_grad_batch(x0, got["U"], op0, ops, ts, W, f, k["kw"]["kind"], u_scale=k["kw"]["u_scale"], figure=figure,
                                      weights=k["kw"]["weights"], reduce=True)
    assert got["cost"] == at["q_mean"]
    assert np.array_equal(got["J"], rc.member_objectives(k, got["U"], figure))
    without = m4q.plant_robust_batch(*k["args"], figure=figure, mem=mem, **k["kw"], **LOOP)
    assert "J" not in without
    _same_run(without, got)


# ---------------------------------------------------------------- 3. against the pure NumPy definition
@pytest.mark.parametrize("mem", [0, 3])
@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_one_call_against_the_numpy_definition(name, figure, mem):
    """Identical decisions; U and cost_hist within 100 times what the definition itself moves when its gradients are pushed by the
    project's gradient bound (tests/plant_robust_cases.py; the host test holds both definition runs to the same decisions).
    Measured on the definition, over the 16 cases: U moved by 1.6e-11 .. 2.2e-08, cost_hist by 8.2e-12 .. 8.9e-10."""
    plain, pushed = rc.definition_runs(name, figure, mem)
    dU, dF = rc.movement(plain, pushed)
    k = rc.parity_case(name)
    got = m4q.plant_robust_batch(*k["args"], figure=figure, mem=mem, iters=rc.PARITY["iters"], steps=rc.PARITY["steps"], step0=rc.STEP0,
                                 tol=0.0, **k["kw"])
    eU, eF = rc.movement(plain, got)
    print("%s %s mem %d: the definition moves U by %.2e, cost_hist by %.2e under the pushed gradient; the device is %.2e, %.2e away"
          % (name, figure, mem, dU, dF, eU, eF))
    assert np.array_equal(got["alpha_hist"], plain["alpha_hist"])
    assert (got["status"], got["n_iter"]) == (plain["status"], plain["n_iter"])
    assert dU > 0 and dF > 0
    assert eU <= 100 * dU and eF <= 100 * dF


# ---------------------------------------------------------------- 4. chaining
@pytest.mark.parametrize("name", ["4-1", "16-1-process"])
def test_three_calls_of_one_iteration_are_one_call_of_three(name):
    k = rc.case(name, 11, 6, 9900 + rc.NAMES.index(name))
    kw = dict(k["kw"], figure="sum", mem=0, steps=4, step0=rc.STEP0, tol=0.0)
    whole = m4q.plant_robust_batch(*k["args"], iters=3, **kw)
    assert whole["status"] == pr.STATUS_ITERS and np.all(whole["alpha_hist"] > 0)
    U = k["args"][1]
    for i in range(3):
        one = m4q.plant_robust_batch(k["args"][0], U, *k["args"][2:], iters=1, **kw)
        assert one["cost_hist"][0] == whole["cost_hist"][i] and one["cost_hist"][1] == whole["cost_hist"][i + 1]
        assert one["alpha_hist"][0] == whole["alpha_hist"][i] and one["pgrad_hist"][0] == whole["pgrad_hist"][i]
        U = one["U"]
    assert np.array_equal(U, whole["U"]) and one["cost"] == whole["cost"]


# ---------------------------------------------------------------- 5. the statuses
def test_statuses_on_the_device():
    k = rc.case("9-2", 5, 5, 9950)
    kw = dict(k["kw"], figure="last", iters=5, steps=4, mem=3, step0=rc.STEP0)
    out = m4q.plant_robust_batch(*k["args"], tol=0.0, gtol=1e6, **kw)                  # 1 by gtol: nothing rolled, nothing moved
    assert (out["status"], out["n_iter"]) == (pr.STATUS_CONVERGED, 1) and out["pgrad_hist"][0] > 0
    assert np.array_equal(out["U"], k["args"][1]) and np.all(out["alpha_hist"] == 0) and np.all(out["cost_hist"] == out["cost"])
    out = m4q.plant_robust_batch(*k["args"], tol=1.0e3, **kw)                          # 1 by tol: the first accepted step ends the run
    assert (out["status"], out["n_iter"]) == (pr.STATUS_CONVERGED, 1) and out["alpha_hist"][0] > 0
    assert out["cost_hist"][1] < out["cost_hist"][0] and np.all(out["cost_hist"][1:] == out["cost"]) and np.all(out["alpha_hist"][1:] == 0)
    args, own = rc.own_trajectory_case()                                               # 2: at its own trajectory no step descends
    out = m4q.plant_robust_batch(*args, members=True, **own)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NO_DESCENT, 1) and 0 < out["cost"] < 1e-15
    assert np.array_equal(out["U"], args[1]) and np.all(out["cost_hist"] == out["cost"]) and np.all(out["alpha_hist"] == 0)
    assert out["J"].shape == (1,) and out["J"][0] == out["cost"]
    bad = args[0].copy()                                                               # 3: the first cost is not finite
    bad[0, 1] = np.nan
    out = m4q.plant_robust_batch(bad, *args[1:], **own)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NOT_FINITE, 0) and np.isnan(out["cost"]) and np.all(np.isnan(out["cost_hist"]))
    assert np.array_equal(out["U"], args[1]) and np.all(out["pgrad_hist"] == 0) and np.all(out["alpha_hist"] == 0)


# ---------------------------------------------------------------- 6. descent on a realistic ensemble
def test_five_iterations_lower_the_mean_of_config_1s_ensemble():
    """Config 1's plant, 64 detuned members, N = 20 (test_projected_gradient_descent_lowers_the_ensemble_mean's setting), through
    QExperiment.robust_batch, with and without the memory.  (Observed on an MI355X from 1.899957: mem = 0 ends at 0.010559,
    mem = 5 at 0.011558 - over five iterations the memory does not pay here, so which run ends lower is printed and not asserted.)"""
    p = configs.build(1)
    B, N = 64, 20
    rng = np.random.default_rng(9950)
    op0 = (1 + 0.2 * rng.standard_normal((B, 1, 1))) * p["plant_op0"][0][None]
    x0 = np.tile(p["x0"][:1], (B, 1))
    exp = m4q.QExperiment(p["plant_op0"][0], list(p["plant_ops"][0]))
    U0 = np.full((N, 1), 0.1 * p["sat"])
    runs = {}
    for mem in (0, 5):
        runs[mem] = exp.robust_batch(x0, U0, p["dt"], p["Qf"].astype(complex), p["X_targ"][:, -1], p["sat"], op0=op0, iters=5, steps=6,
                                     mem=mem, step0=0.5 * p["sat"], tol=0.0)
        h = runs[mem]["cost_hist"]
        print("mem %d: cost %s, alpha %s" % (mem, np.array2string(h, precision=6), runs[mem]["alpha_hist"]))
        assert runs[mem]["cost"] < h[0] and np.all(np.diff(h) <= 0) and np.all(np.abs(runs[mem]["U"]) <= p["sat"])
    assert np.array_equal(runs[5]["cost_hist"][:2], runs[0]["cost_hist"][:2])          # (the first step is the memoryless one in both)

"""The robust optimiser on models on the device (m4q_model_robust_batch) and the kernel its line search runs on
(model_rollout_multi_kernel, m4q_model_rollout_multi_batch): the multi rollout against model_rollout_batch and
ordered_weighted_sum bit for bit at every built model shape - the shapes that keep the model's rows in registers and the ones
that read them from LDS at every step; the one call against the definition driven by the package's earlier device entry points,
bit for bit; against the pure NumPy definition with a bound measured on the definition itself; chaining; the statuses; a
dissipative qubit end to end, judged on the generator plant's own rollout.

Shapes are the smallest that can go wrong: B = 7 and 11 (ragged quads), N = 5 and 6; B = 259 for the reduction (two chunks, the
second ragged); one case with 4,098 quads, past the grid the launch is capped at."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd import plant_robust as pr
from mpc4quantum_amd.configs import I2, SX, SY, SZ
from mpc4quantum_amd.csrc import build as hip_build
from tests import model_robust_cases as mc
from tests import plant_robust_cases as rc

pytestmark = pytest.mark.gpu

# every object with model kernels: m4q_shapes.inc without its plant-only lines, as the build reads it
BUILT = [(nx, nu, order) for nx, nu, order, plant_only in hip_build.shapes() if not plant_only]


# ---------------------------------------------------------------- 1. the multi kernel
def _random_models(rng, B, n, m, order):
    """Per-member models near the identity: nothing in the kernel depends on where a model came from."""
    P = m4q.size_of_library(order, m) - 1
    mdl = 0.15 * (rng.standard_normal((B, n, n * (1 + P))) + 1j * rng.standard_normal((B, n, n * (1 + P)))) / np.sqrt(n)
    mdl[:, :, :n] += np.eye(n)
    return mdl


def _multi_case(shape, B, N, seed):
    n, m, order = shape
    rng = np.random.default_rng(seed)
    models = _random_models(rng, B, n, m, order)
    x0 = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    sc = 1 + 0.1 * rng.standard_normal((B, m))
    W = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    f = 0.3 * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    w = rng.uniform(0.5, 1.5, B)
    return dict(shape=shape, args=(x0, None, models, order, W, f, 0.6), kw=dict(u_scale=sc, weights=w / w.sum())), rng


def _multi_check(shape, B, N, S, figure, weighted, per_member, seed):
    k, rng = _multi_case(shape, B, N, seed)
    x0, _, models, order, W, f, sat = k["args"]
    if not per_member:
        models = models[B // 2]
        k["args"] = (x0, None, models, order, W, f, sat)
    us = rng.uniform(-sat, sat, (S, N, shape[1]))
    kw = dict(k["kw"], figure=figure)
    if not weighted:
        kw["weights"] = None
    out = m4q.model_rollout_multi_batch(x0, us, models, order, W, f, **kw)
    assert out["J"].shape == (B, S) and out["F"].shape == (S,) and np.isfinite(out["J"]).all()
    for s in range(S):
        assert np.array_equal(out["J"][:, s], mc.member_objectives(k, us[s], figure)), (shape, s)
    assert np.array_equal(out["F"], m4q.ordered_weighted_sum(out["J"], kw["weights"]))
    again = m4q.model_rollout_multi_batch(x0, us, models, order, W, f, **kw)
    assert np.array_equal(again["J"], out["J"]) and np.array_equal(again["F"], out["F"])
    # each output alone is the same output
    only_F = m4q.model_rollout_multi_batch(x0, us, models, order, W, f, members=False, **kw)
    only_J = m4q.model_rollout_multi_batch(x0, us, models, order, W, f, mean=False, **kw)
    assert set(only_F) == {"F"} and set(only_J) == {"J"}
    assert np.array_equal(only_F["F"], out["F"]) and np.array_equal(only_J["J"], out["J"])
    assert np.ptp(out["J"], axis=0).min() > 0 and (S == 1 or np.ptp(out["F"]) > 0)          # (members and sequences differ)


@pytest.mark.parametrize("per_member", [True, False], ids=["per-member", "shared"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "uniform"])
@pytest.mark.parametrize("figure", ["last", "sum"])
@pytest.mark.parametrize("shape", BUILT, ids=str)
def test_multi_rollout_equals_the_rollout_and_the_ordered_sum(shape, figure, weighted, per_member):
    _multi_check(shape, 7, 5, 3, figure, weighted, per_member, 9600 + 7 * BUILT.index(shape))


def test_every_built_model_shape_has_the_kernel():
    """(The list above is the build's own; both forms of the kernel are in it, and a shape the library lacks would fail here.)"""
    assert len(BUILT) >= 11 and (9, 2, 1) in BUILT and (9, 2, 2) in BUILT and (16, 2, 1) not in BUILT
    for nx, nu, order in BUILT:
        assert _lib.lib().m4q_supported(nx, nu, order) == 1, (nx, nu, order)


@pytest.mark.parametrize("B,N,S", [(7, 5, 1), (7, 5, 8), (259, 5, 3), (16389, 5, 2)], ids=str)
def test_multi_rollout_at_the_edges_of_s_the_chunks_and_the_grid(B, N, S):
    _multi_check((4, 1, 1), B, N, S, "sum", True, True, 9700 + S)


# ---------------------------------------------------------------- 2. the one call against the definition driven by the device
LOOP = dict(iters=mc.PARITY["iters"], steps=mc.PARITY["steps"], step0=rc.STEP0, tol=0.0)
HISTORY = ("U", "cost_hist", "alpha_hist", "pgrad_hist")


def _same_run(got, want):
    for key in HISTORY:
        assert np.array_equal(got[key], want[key]), key
    assert (got["cost"], got["n_iter"], got["status"]) == (want["cost"], want["n_iter"], want["status"])


@pytest.mark.parametrize("mem", mc.MEMS)
@pytest.mark.parametrize("figure", mc.FIGURES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_one_call_equals_the_definition_on_the_device_entry_points(shape, figure, mem):
    k = mc.parity_case(shape, figure, mem)
    x0, _, models, order, W, f, _ = k["args"]
    want = m4q.plant_robust_reference(None, k["args"][1], None, None, None, None, None, k["args"][6], mem=mem,
                                      evaluate=mc.device_evaluate(k, figure), **LOOP)
    got = m4q.model_robust_batch(*k["args"], figure=figure, mem=mem, members=True, **k["kw"], **LOOP)
    _same_run(got, want)
    assert np.count_nonzero(got["alpha_hist"]) >= 2 and got["cost"] < got["cost_hist"][0]
    at = m4q.model_rollout_grad_batch(x0, got["U"], models, order, W, f, u_scale=k["kw"]["u_scale"], figure=figure,
                                      weights=k["kw"]["weights"], reduce=True)
    assert got["cost"] == at["q_mean"]
    assert np.array_equal(got["J"], mc.member_objectives(k, got["U"], figure))
    without = m4q.model_robust_batch(*k["args"], figure=figure, mem=mem, **k["kw"], **LOOP)
    assert "J" not in without
    _same_run(without, got)


# ---------------------------------------------------------------- 3. against the pure NumPy definition
@pytest.mark.parametrize("mem", mc.MEMS)
@pytest.mark.parametrize("figure", mc.FIGURES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=str)
def test_one_call_against_the_numpy_definition(shape, figure, mem):
    """Identical decisions; U and cost_hist within 100 times what the definition itself moves when its gradients are pushed by the
    project's gradient bound, 1e-10 max(1, max|g|) (tests/model_robust_cases.py; the host test holds both definition runs to the
    same decisions).  The movement is computed here, on the definition, not taken from a constant: over the 20 cells U moves by
    1.8e-11 .. 8.0e-09 and cost_hist by 7.1e-12 .. 8.2e-09."""
    plain, pushed = mc.definition_runs(shape, figure, mem)
    dU, dF = rc.movement(plain, pushed)
    k = mc.parity_case(shape, figure, mem)
    got = m4q.model_robust_batch(*k["args"], figure=figure, mem=mem, iters=mc.PARITY["iters"], steps=mc.PARITY["steps"], step0=rc.STEP0,
                                 tol=0.0, **k["kw"])
    eU, eF = rc.movement(plain, got)
    print("%s %s mem %d: the definition moves U by %.2e, cost_hist by %.2e under the pushed gradient; the device is %.2e, %.2e away"
          % (shape, figure, mem, dU, dF, eU, eF))
    assert np.array_equal(got["alpha_hist"], plain["alpha_hist"])
    assert (got["status"], got["n_iter"]) == (plain["status"], plain["n_iter"])
    assert dU > 0 and dF > 0
    assert eU <= 100 * dU and eF <= 100 * dF


# ---------------------------------------------------------------- 4. chaining
@pytest.mark.parametrize("shape", [(4, 1, 1), (9, 2, 2)], ids=str)
def test_three_calls_of_one_iteration_are_one_call_of_three(shape):
    k = mc.case(shape, 11, 6, 9900 + shape[0])
    kw = dict(k["kw"], figure="sum", mem=0, steps=4, step0=rc.STEP0, tol=0.0)
    whole = m4q.model_robust_batch(*k["args"], iters=3, **kw)
    assert whole["status"] == pr.STATUS_ITERS and np.all(whole["alpha_hist"] > 0)
    U = k["args"][1]
    for i in range(3):
        one = m4q.model_robust_batch(k["args"][0], U, *k["args"][2:], iters=1, **kw)
        assert one["cost_hist"][0] == whole["cost_hist"][i] and one["cost_hist"][1] == whole["cost_hist"][i + 1]
        assert one["alpha_hist"][0] == whole["alpha_hist"][i] and one["pgrad_hist"][0] == whole["pgrad_hist"][i]
        U = one["U"]
    assert np.array_equal(U, whole["U"]) and one["cost"] == whole["cost"]


# ---------------------------------------------------------------- 5. the statuses
def test_statuses_on_the_device():
    k = mc.case((8, 2, 1), 5, 5, 9950)
    kw = dict(k["kw"], figure="last", iters=5, steps=4, mem=3, step0=rc.STEP0)
    out = m4q.model_robust_batch(*k["args"], tol=0.0, gtol=1e6, **kw)                  # 1 by gtol: nothing rolled, nothing moved
    assert (out["status"], out["n_iter"]) == (pr.STATUS_CONVERGED, 1) and out["pgrad_hist"][0] > 0
    assert np.array_equal(out["U"], k["args"][1]) and np.all(out["alpha_hist"] == 0) and np.all(out["cost_hist"] == out["cost"])
    out = m4q.model_robust_batch(*k["args"], tol=1.0e3, **kw)                          # 1 by tol: the first accepted step ends the run
    assert (out["status"], out["n_iter"]) == (pr.STATUS_CONVERGED, 1) and out["alpha_hist"][0] > 0
    assert out["cost_hist"][1] < out["cost_hist"][0] and np.all(out["cost_hist"][1:] == out["cost"]) and np.all(out["alpha_hist"][1:] == 0)
    args, own = mc.own_trajectory_case()                                               # 2: at its own trajectory no step descends
    out = m4q.model_robust_batch(*args, members=True, **own)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NO_DESCENT, 1) and 0 < out["cost"] < 1e-15
    assert np.array_equal(out["U"], args[1]) and np.all(out["cost_hist"] == out["cost"]) and np.all(out["alpha_hist"] == 0)
    assert out["J"].shape == (1,) and out["J"][0] == out["cost"]
    bad = args[0].copy()                                                               # 3: the first cost is not finite
    bad[0, 1] = np.nan
    out = m4q.model_robust_batch(bad, *args[1:], **own)
    assert (out["status"], out["n_iter"]) == (pr.STATUS_NOT_FINITE, 0) and np.isnan(out["cost"]) and np.all(np.isnan(out["cost_hist"]))
    assert np.array_equal(out["U"], args[1]) and np.all(out["pgrad_hist"] == 0) and np.all(out["alpha_hist"] == 0)


# ---------------------------------------------------------------- 6. dissipative dynamics, end to end
def test_a_dissipative_ensemble_end_to_end():
    """QExperiment with a collapse operator: robust_model_batch discretises the members' Lindblad generators on the device
    (order 2), optimises one pulse on the models, and the pulse is judged on the generator plant's own rollout.  The run takes the
    decisions of the NumPy definition on the same models."""
    c, d = mc.dissipative_case(), mc.DISSIPATIVE
    loop = dict(iters=d["iters"], steps=d["steps"], mem=d["mem"], step0=d["step0"], tol=d["tol"])
    out = c["exp"].robust_model_batch(c["x0"], c["U0"], d["dt"], 2, c["W"], c["target"], d["sat"], op0=c["L0"], u_scale=c["u_scale"],
                                      figure="last", **loop)
    assert out["models"].shape == (d["B"], 4, 4 * 3)
    host = m4q.discretize_homogeneous([c["L0"], np.broadcast_to(c["L1"], c["L0"].shape)], d["dt"], 2)
    assert np.abs(out["models"] - host).max() <= 1e-14

    def plant_mean(U):
        q = m4q.plant_rollout_batch(c["x0"], U, c["L0"], c["L1"][None], d["dt"], _lib.PLANT_GENERATOR, u_scale=c["u_scale"], W=c["W"],
                                    target=c["target"], keep="none", figure="last")["q"]
        return float(m4q.ordered_weighted_sum(q))
    before, after = plant_mean(c["U0"]), plant_mean(out["U"])
    print("the model mean goes %.3f -> %.3f, the generator plant's %.3f -> %.3f" % (out["cost_hist"][0], out["cost"], before, after))
    assert after < before and np.all(np.diff(out["cost_hist"]) <= 0) and np.all(np.abs(out["U"]) <= d["sat"])
    assert abs(before - mc.generator_plant_mean(c, c["U0"])) <= 1e-9 and abs(after - mc.generator_plant_mean(c, out["U"])) <= 1e-9
    ref = m4q.model_robust_reference(c["x0"], c["U0"], out["models"], 2, c["W"], c["target"], d["sat"], u_scale=c["u_scale"],
                                     figure="last", **loop)
    assert np.array_equal(out["alpha_hist"], ref["alpha_hist"]) and (out["status"], out["n_iter"]) == (ref["status"], ref["n_iter"])


# ---------------------------------------------------------------- 7. every route of robust_model_batch
def _route(name):
    """(experiment, n, order, per-member op0 or None, the generators the models must come from)"""
    rng = np.random.default_rng(9990)
    B = 6
    xi = 1 + 0.05 * rng.standard_normal(B)
    if name == "hamiltonian-per-member-order-2":                     # liouvillian of a [B, d, d] op0, discretised on the device
        H0, H1 = 0.15 * SZ, 0.5 * SX
        op0 = xi[:, None, None] * H0
        return m4q.QExperiment(H0, [H1]), 4, 2, op0, [m4q.liouvillian(op0), np.broadcast_to(m4q.liouvillian(H1), (B, 4, 4))]
    if name == "hamiltonian-shared-order-1":                         # op0 None: one shared model [n, n (1 + P)]
        H0, H1 = 0.15 * SZ, 0.5 * SX
        return m4q.QExperiment(H0, [H1]), 4, 1, None, [m4q.liouvillian(H0), m4q.liouvillian(H1)]
    assert name == "generators-per-member-order-3"                   # LExperiment: generators as they stand, discretised on the host
    L0, L1 = m4q.liouvillian(np.kron(SZ, SZ)), m4q.liouvillian(np.kron(SY, I2))
    op0 = xi[:, None, None] * L0
    return m4q.LExperiment(L0, [L1]), 16, 3, op0, [op0, np.broadcast_to(L1, (B, 16, 16))]


@pytest.mark.parametrize("name", ["hamiltonian-per-member-order-2", "hamiltonian-shared-order-1", "generators-per-member-order-3"])
def test_robust_model_batch_discretises_the_right_generators_and_optimises_on_them(name):
    exp, n, order, op0, gens = _route(name)
    B, N, dt, sat = 6, 6, 0.25, 2 * np.pi * 0.1
    rng = np.random.default_rng(9991)
    x0 = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    x0 /= np.linalg.norm(x0, axis=1, keepdims=True)
    W, f = np.eye(n, dtype=complex), 0.3 * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    U0 = rng.uniform(-0.5 * sat, 0.5 * sat, (N, 1))
    sc = 1 + 0.02 * rng.standard_normal((B, 1))
    loop = dict(iters=3, steps=4, mem=3, step0=rc.STEP0, tol=0.0)
    out = exp.robust_model_batch(x0, U0, dt, order, W, f, sat, op0=op0, u_scale=sc, figure="sum", members=True, **loop)
    host = m4q.discretize_homogeneous(gens, dt, order)
    assert out["models"].shape == host.shape == ((B, n, host.shape[-1]) if op0 is not None else (n, host.shape[-1]))
    assert np.abs(out["models"] - host).max() <= (1e-14 if order <= 2 else 0.0)
    direct = m4q.model_robust_batch(x0, U0, out["models"], order, W, f, sat, u_scale=sc, figure="sum", members=True, **loop)
    _same_run(out, direct)
    assert np.array_equal(out["J"], direct["J"]) and out["cost"] < out["cost_hist"][0] and np.count_nonzero(out["alpha_hist"]) >= 2

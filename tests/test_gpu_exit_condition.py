"""Exit conditions evaluated by the closed-loop kernel (QuadraticExit, m4q_session_set_exit): the drop-in mpc() against the
reference's own runs in one launch, planned exits on every compiled kernel variant with a device plant, measure_freq = 2, resumed
launches, and a detuned synthesis ensemble against the condition recomputed on the host."""
import os
import warnings

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from mpc4quantum_amd.mpc import open_session
from tests import kernel_variants as kv
from tests.kernel_variants import _check_planned, _planned
from tests.test_gpu_synthesis import _case, _check_vs_reference, _dropin
from tests.test_gpu_variant_matrix import _open, _scenario

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


@pytest.fixture
def count_runs(monkeypatch):
    calls = []
    orig = m4q.EnsembleSession.run

    def run(self, *a, **k):
        calls.append(a)
        return orig(self, *a, **k)
    monkeypatch.setattr(m4q.EnsembleSession, "run", run)
    return calls


# ---------------------------------------------------------------- 1. drop-in mpc() against the reference, fused
@pytest.mark.parametrize("name", ["o1_exit", "o2_exit", "o3_exit", "o4_exit", "o1_exit_mid", "o3_exit_mid"])
def test_mpc_dropin_quadratic_exit_fused_vs_reference(count_runs, name):
    """The synthesis test's condition ((p1 - pf)^H Q (p1 - pf)).real < thr as a QuadraticExit: one launch, the reference's result."""
    g = np.load(os.path.join(GOLDEN, "synthesis.npz"))
    c = _case(g, name)
    cond = m4q.QuadraticExit(g["not_Q"], g["not_pf"], float(c["exit_thr"]), state="prev", fires="below")
    xs, us, code, clock = _dropin(g, c, exit_condition=cond, qp_flags=_lib.QP_REF_LQR)
    assert len(count_runs) == 1
    _check_vs_reference(xs, us, code, clock, c)


@pytest.mark.parametrize("name", ["qubit_o1_exit_step3", "qubit_o1_exit_step0"])
def test_mpc_dropin_abs_exit_fused_vs_reference(count_runs, name):
    """abs(x_next[i]) > t as W = e_i e_i^T, f = 0, 'next', 'above', thr = t^2: code 1, the dropped entry, us None at step 0."""
    from tests.test_gpu_parity import _ref_plant
    g = np.load(os.path.join(GOLDEN, "mpc_loop.npz"))
    k = "loop_" + name + "_"
    c = {key[len(k):]: g[key] for key in g.files if key.startswith(k)}
    n, i, t = int(c["d"]) ** 2, int(c["exit_index"]), float(c["exit_thr"])
    W = np.zeros((n, n))
    W[i, i] = 1.0
    cond = m4q.QuadraticExit(W, np.zeros(n), t * t if t >= 0 else -1.0, state="next", fires="above")
    model = m4q.DMDc(n, n, c["model"].shape[1] - n, c["model"])
    clock = m4q.StepClock(float(c["dt"]), int(c["T"]), int(c["n_steps"]))
    clock.measure_freq = int(c["measure_freq"])
    cc = dict(c, growth=float(c["growth"]), d=int(c["d"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (xs, us), _, code = m4q.mpc(c["x0"], int(c["m"]), int(c["order"]), c["X_targ"], c["U_targ"], clock, _ref_plant(cc), model,
                                    c["Q"], c["R"], c["Q"], sat=float(c["sat"]), du=float(c["du"]), max_iter=int(c["max_iter"]),
                                    exit_condition=cond, warm_start=bool(c["warm_start"]), progress_bar=False,
                                    qp_flags=_lib.QP_REF_LQR)
    assert len(count_runs) == 1
    assert code == 1 == int(c["exit_code"]) and xs.shape == c["xs"].shape
    assert rel(xs, c["xs"]) <= 1e-9
    if bool(c["us_is_none"]):
        assert us is None
    else:
        assert us.shape == c["us"].shape and rel(us, c["us"]) <= 1e-9
    assert np.array_equal(clock.ts_sim, c["ts_sim"])


# ---------------------------------------------------------------- 2. planned exits on every kernel variant with a device plant
PLANT_CELLS = [c for c in kv.closed_loop_cells() if c.plant != kv.NONE]


def _results(sess):
    r = sess.results()
    return {k: r[k].copy() for k in ("xs", "us", "exit_codes", "steps_done", "qp_solves")}


@pytest.mark.parametrize("cell", PLANT_CELLS, ids=kv.cell_id)
def test_planned_exits_every_plant_cell(cell):
    """Targets equal to each member's own stored state at a planned step, thr 1e-30 below: code 1 and steps_done at exactly the
    first step whose stored state equals the target, the run up to it bit-identical to the run without a condition, members that
    never meet it bit-identical throughout; both 'prev' and 'next'."""
    p = _scenario(cell)
    ns, n = p["n_steps"], p["dim_x"]
    sess = _open(cell, p)
    try:
        assert sess.path_detail() == cell.path
        sess.run(0, ns)
        ref = _results(sess)
        assert np.all(ref["exit_codes"] == 0)
        fired = 0
        for state in ("prev", "next"):
            target = _planned(ref["xs"], state, ns)
            sess.set_exit_condition(m4q.QuadraticExit(np.identity(n), target, 1e-30, state=state, fires="below"))
            sess.run(0, ns)
            got = _results(sess)
            _check_planned(ref, got, target, state, ns)
            fired += int(np.sum(got["exit_codes"] == 1))
        assert fired >= 2 * (p["batch"] - 2)
        sess.set_exit_condition(None)
        sess.run(0, ns)
        again = _results(sess)
        for f in ref:
            assert np.array_equal(again[f], ref[f]), f
    finally:
        sess.close()


# ---------------------------------------------------------------- 3. measure_freq = 2
def test_planned_exits_measure_freq_2():
    """Every other step closes the loop through the model: 'next' sees the model's prediction stored there."""
    p = configs.build(2, batch=9, horizon=8, n_steps=6)
    ns, n = p["n_steps"], p["dim_x"]
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    clock.measure_freq = 2
    args = (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
            p["R"], p["Qf"], p["sat"], p["du"])
    sess = open_session(*args)
    try:
        sess.run(0, ns)
        ref = _results(sess)
        assert np.all(ref["exit_codes"] == 0)
        for state in ("prev", "next"):
            target = _planned(ref["xs"], state, ns)
            sess.set_exit_condition(m4q.QuadraticExit(np.identity(n), target, 1e-30, state=state))
            sess.run(0, ns)
            got = _results(sess)
            _check_planned(ref, got, target, state, ns)
            assert np.sum(got["exit_codes"] == 1) >= p["batch"] - 3
    finally:
        sess.close()


# ---------------------------------------------------------------- 4. resumed launches; set then clear
@pytest.mark.parametrize("cell", [c for c in PLANT_CELLS if c.path == kv.COMPLEX and c.order == 1 and not c.exact], ids=kv.cell_id)
def test_exit_condition_resumed_launch_bit_identical(cell):
    """run(0, k) then run(k, ns) with a condition set equals one launch bit for bit (the complex path: a resumed launch of the real
    paths changes basis once more, test_gpu_parity.py::test_checkpoint_resume), members that exited in the first launch stay at
    code 1; clearing the condition gives the unconditioned results again."""
    p = _scenario(cell)
    ns, n = p["n_steps"], p["dim_x"]
    sess = _open(cell, p)
    try:
        sess.run(0, ns)
        ref = _results(sess)
        target = _planned(ref["xs"], "next", ns)
        sess.set_exit_condition(m4q.QuadraticExit(np.identity(n), target, 1e-30, state="next"))
        sess.run(0, ns)
        one = _results(sess)
        for k in range(1, ns):
            sess.run(0, k)
            mid = _results(sess)
            sess.run(k, ns)
            two = _results(sess)
            for f in one:
                assert np.array_equal(two[f], one[f]), (k, f)
            early = mid["exit_codes"] == 1
            assert np.all(two["exit_codes"][early] == 1) and np.array_equal(two["steps_done"][early], mid["steps_done"][early])
        sess.set_exit_condition(None)
        sess.run(0, ns)
        cleared = _results(sess)
        for f in ref:
            assert np.array_equal(cleared[f], ref[f]), f
    finally:
        sess.close()


# ---------------------------------------------------------------- 5. a detuned synthesis ensemble
def test_synthesis_ensemble_exit_matches_host_recompute():
    """4,093 detuned NOT-gate members, the synthesis test's condition with a threshold about half of them reach: every member's
    code 1 at step s is the first step whose stored state meets the condition recomputed on the host; the others run to the end."""
    p = configs.synthesis(4093, 1, detuning_spread=0.3)
    ns, B = p["n_steps"], p["batch"]
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    args = (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
            p["R"], p["Qf"], p["sat"], p["du"])
    kw = dict(plant_kind=_lib.PLANT_PROCESS)
    ref = m4q.mpc_batch(*args, **kw)
    assert np.all(ref["exit_codes"] == 0)
    Wq, pf = np.asarray(p["Q"], dtype=complex), p["target"]
    d = np.swapaxes(ref["xs"], 1, 2)[:, :ns] - pf                                     # [B, ns, n]: xs[s] of every step s
    q = np.einsum("bsi,ij,bsj->bs", d.conj(), Wq, d).real
    thr = float(np.median(q.min(axis=1)))
    cond = m4q.QuadraticExit(Wq, pf, thr, state="prev", fires="below")
    got = m4q.mpc_batch(*args, exit_condition=cond, **kw)
    checked = fired = 0
    for b in range(B):
        hit = np.nonzero(q[b] < thr)[0]
        s = int(hit[0]) if hit.size else ns
        if np.any(np.abs(q[b, :min(s + 1, ns)] - thr) <= 1e-12 * thr):
            continue
        checked += 1
        if hit.size:
            fired += 1
            assert got["exit_codes"][b] == 1 and got["steps_done"][b] == s, (b, s, got["exit_codes"][b], got["steps_done"][b])
            assert np.array_equal(got["xs"][b][:, :s + 1], ref["xs"][b][:, :s + 1])
        else:
            assert got["exit_codes"][b] == 0 and got["steps_done"][b] == ns
    assert checked >= B - 10 and B // 4 <= fired <= 3 * B // 4

"""Gate synthesis on the device (M4Q_PLANT_PROCESS, shapes (16, 1, 1-4)): the process plant kernel, the drop-in mpc() with
QSynthesis against the reference's own mpc.py (tests/golden/synthesis.npz), ensembles of detuned plants against the oracle,
the forced complex path, and the exact box-QP mode against BVLS."""
import os

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from oracle import m4q_oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthesis.npz")
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def process_step(P, u, H0, Hs, dt):
    from scipy.linalg import expm
    H = H0 + sum(float(uk) * h for uk, h in zip(u, Hs))
    V = expm(-1j * dt * H)
    return (np.kron(V, V.conj()) @ np.reshape(P, (4, 4))).reshape(-1)


def process_generators(Hs):
    eye = np.identity(2)
    return np.stack([np.kron(-1j * (np.kron(h, eye) - np.kron(eye, h.conj())), np.identity(4)) for h in Hs])


def _case(g, name):
    k = "not_%s_" % name
    return {key[len(k):]: g[key] for key in g.files if key.startswith(k)}


# ---------------------------------------------------------------- 1. the plant kernel
def test_process_plant_step_ragged_batch():
    """4,097 members (one past a multiple of the four rows of a wavefront), per-member H0: the device's process step equals the
    NumPy step (V (x) V^*) M and the device's own generator plant on L (x) I_4, both to 1e-13."""
    rng = np.random.default_rng(21)
    B, dt = 4097, 0.05
    H0 = rng.standard_normal((B, 2, 2)) + 1j * rng.standard_normal((B, 2, 2))
    H0 = 0.5 * (H0 + np.swapaxes(H0.conj(), 1, 2))
    Hk = np.stack([0.5 * SX])
    U = np.linalg.qr(rng.standard_normal((B, 2, 2)) + 1j * rng.standard_normal((B, 2, 2)))[0]
    x = np.einsum('bij,bkl->bikjl', U, U.conj()).reshape(B, 16)
    x[B // 2:] += 0.1 * (rng.standard_normal((B - B // 2, 16)) + 1j * rng.standard_normal((B - B // 2, 16)))  # general M too
    u = rng.uniform(-1, 1, (B, 1))
    got = m4q.plant_step_batch(x, u, H0, Hk[None], dt, _lib.PLANT_PROCESS)
    ref = np.stack([process_step(x[b], u[b], H0[b], list(Hk), dt) for b in range(B)])
    assert np.abs(got - ref).max() <= 1e-13
    L = np.stack([process_generators([H0[b]] + list(Hk)) for b in range(B)])
    gen = m4q.plant_step_batch(x, u, L[:, 0], L[:, 1:], dt, _lib.PLANT_GENERATOR)
    assert np.abs(got - gen).max() <= 1e-13
    # the shared-operator form (plant_per_instance = 0)
    got1 = m4q.plant_step_batch(x[:5], u[:5], H0[0], Hk, dt, _lib.PLANT_PROCESS)
    assert np.abs(got1 - np.stack([process_step(x[b], u[b], H0[0], list(Hk), dt) for b in range(5)])).max() <= 1e-13


def test_process_plant_refuses_bad_shapes():
    x = np.zeros((3, 16), dtype=complex)
    u = np.zeros((3, 1))
    with pytest.raises(ValueError):                                   # operators of the HAMILTONIAN plant's size (4 x 4)
        m4q.plant_step_batch(x, u, np.zeros((4, 4)), np.zeros((1, 4, 4)), 0.1, _lib.PLANT_PROCESS)
    with pytest.raises(ValueError):
        m4q.plant_step_batch(x, u, np.zeros((2, 2)), np.zeros((2, 2, 2)), 0.1, _lib.PLANT_PROCESS)
    L = _lib.lib()
    for n, m in ((9, 2), (4, 1), (8, 2)):                             # not a fourth power: M4Q_E_BADARG from the C ABI
        xb = np.zeros((1, n), dtype=complex)
        out = np.zeros_like(xb)
        op = np.zeros(64, dtype=complex)
        rc = L.m4q_plant_step_batch(1, n, m, _lib.PLANT_PROCESS, 0.1, _lib.cbuf(xb)[1], _lib.rbuf(np.zeros((1, m)))[1],
                                    _lib.cbuf(op)[1], _lib.cbuf(op)[1], 0, out.ctypes.data_as(_lib._dp))
        assert rc == _lib.E_BADARG, (n, rc)
    for n, m, order in ((9, 2, 1), (8, 2, 1)):
        with pytest.raises(_lib.M4qError) as e:
            m4q.EnsembleSession(1, n, m, order, 4, 2, 0.1, 1.0, plant_kind=_lib.PLANT_PROCESS)
        assert e.value.code == _lib.E_BADARG


def test_device_discretisation_refuses_orders_3_4():
    p = configs.synthesis(2, 3)
    sess = m4q.EnsembleSession(2, 16, 1, 3, p["horizon"], 2, p["dt"], p["sat"], p["du"], plant_kind=_lib.PLANT_PROCESS,
                               model_per_instance=True, target_cols=p["n_steps"] + p["horizon"] + 1)
    try:
        with pytest.raises(_lib.M4qError, match="orders 1 and 2"):
            sess.build_models(p["dt"], p["generators"])
    finally:
        sess.close()
    with pytest.raises(_lib.M4qError, match="orders 1 and 2"):
        m4q.discretize_homogeneous_batch(list(p["generators"]), p["dt"], 4)


# ---------------------------------------------------------------- 2. drop-in mpc() against the reference's mpc.py
def _dropin(g, c, exit_condition=None, **kw):
    order = int(c["order"])
    Hp = list(c["H_plant"])
    exp = m4q.QSynthesis(Hp[0], Hp[1:])
    model = m4q.DMDc(16, 16, c["model"].shape[1] - 16, c["model"])
    clock = m4q.StepClock(float(g["not_dt"]), int(g["not_T"]), int(g["not_n_steps"]))
    (xs, us), _, code = m4q.mpc(g["not_p0"], 1, order, g["not_X_targ"], g["not_U_targ"], clock, exp, model, g["not_Q"], g["not_R"],
                                g["not_Qf"], sat=float(g["not_sat"]), du=float(g["not_du"]), exit_condition=exit_condition,
                                progress_bar=False, **kw)
    return xs, us, code, clock


def _check_vs_reference(xs, us, code, clock, c):
    """Exit code, shapes, ts_sim; MPC steps 0 and 1 to 1e-10, every step to 1e-9 - each plus 100 times what the REFERENCE's own run
    moves when P0 is scaled by 1 +- 1e-14 (env_*, running maximum: at order 1 the reference's loop chatters between the bounds,
    and the detuned order-1 run already moves by 1e-8 in its control of step 1)."""
    assert code == int(c["exit_code"]) and xs.shape == c["xs"].shape
    assert np.array_equal(clock.ts_sim, c["ts_sim"])
    env_x = c["env_xs"]
    assert np.all(np.abs(xs[:, :3] - c["xs"][:, :3]).max(axis=0) <= 1e-10 + 100 * env_x[:3])
    assert np.all(np.abs(xs - c["xs"]).max(axis=0) <= 1e-9 + 100 * env_x), np.abs(xs - c["xs"]).max(axis=0)
    if bool(c["us_is_none"]):
        assert us is None
        return
    env_u = c["env_us"]
    assert us.shape == c["us"].shape
    assert np.all(np.abs(us[:, :2] - c["us"][:, :2]).max(axis=0) <= 1e-10 + 100 * env_u[:2])
    assert np.all(np.abs(us - c["us"]).max(axis=0) <= 1e-9 + 100 * env_u), np.abs(us - c["us"]).max(axis=0)


@pytest.mark.parametrize("name", ["o1", "o2", "o3", "o4", "o1_detuned", "o2_detuned"])
def test_mpc_dropin_fused_vs_reference_mpc_py(g, name):
    """No exit_condition: the fused path (one launch, process plant on the device), QP_REF_LQR (lqr.py's arithmetic)."""
    c = _case(g, name)
    xs, us, code, clock = _dropin(g, c, qp_flags=_lib.QP_REF_LQR)
    _check_vs_reference(xs, us, code, clock, c)


@pytest.mark.parametrize("name", ["o1_exit", "o2_exit", "o3_exit", "o4_exit", "o1_exit_mid", "o3_exit_mid"])
def test_mpc_dropin_host_path_exit_condition_vs_reference_mpc_py(g, name):
    """With the test's exit_condition (tests/test_mpc4quantum.py:100-101; threshold 1e-2, never met, or 7.9, met mid-run): the
    host path, one launch per MPC step with QSynthesis.simulate stepping the process vector on the device."""
    c = _case(g, name)
    pf, Q, thr = g["not_pf"], g["not_Q"], float(c["exit_thr"])

    def exit_condition(p2, p1, u1):
        return ((p1 - pf).conj().T @ Q @ (p1 - pf)).real < thr
    xs, us, code, clock = _dropin(g, c, exit_condition=exit_condition, qp_flags=_lib.QP_REF_LQR)
    _check_vs_reference(xs, us, code, clock, c)


# ---------------------------------------------------------------- 3. ensembles of detuned plants
def test_ensemble_detuned_vs_oracle_teacher_forced():
    """4,093 members (ragged on purpose), per-member detunings of the plant, one nominal model: the complex path; sampled
    members teacher-forced against oracle.mpc (qp_mode "qp") step by step - us[k], xs[k+1] to 1e-10, the guesses left behind to
    1e-7 (or ten times what the oracle moves under a 1e-15 perturbation of the guess its step starts from); every member's result
    bit-identical to its own single-member run."""
    B, ns = 4093, 12
    p = configs.synthesis(B, 2, detuning_spread=0.3, n_steps=ns)
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    res = m4q.mpc_batch(p["x0"], p["models"], 1, 2, p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
                        p["R"], p["Qf"], p["sat"], p["du"], plant_kind=_lib.PLANT_PROCESS)
    assert res["path"] == "complex" and res["path_detail"] == "complex"
    assert np.all(res["exit_codes"] == 0) and np.all(res["steps_done"] == ns)
    assert np.abs(res["us"]).max() <= p["sat"] * (1 + 1e-15)
    sample = [0, 1, 2, 3, 2047, B - 2, B - 1]
    # single-member runs: bit-identical
    for b in sample[::3]:
        one = m4q.mpc_batch(p["x0"][b:b + 1], p["models"], 1, 2, p["X_targ"], p["U_targ"], m4q.StepClock(p["dt"], p["horizon"], ns),
                            p["plant_op0"][b:b + 1], p["plant_ops"], p["Q"], p["R"], p["Qf"], p["sat"], p["du"],
                            plant_kind=_lib.PLANT_PROCESS)
        assert np.array_equal(one["xs"][0], res["xs"][b]) and np.array_equal(one["us"][0], res["us"][b])
        assert np.array_equal(one["qp_solves"][0], res["qp_solves"][b])
    # teacher forcing: the oracle's run of each sampled member, and a session of those members restarted from it at every step
    n, m, T = 16, 1, p["horizon"]
    model = orc.OracleDMDc(n, n, p["models"].shape[2] - n, p["models"][0])
    runs = []
    for b in sample:
        L = process_generators([p["plant_op0"][b], p["plant_ops"][0, 0]])
        exp = orc.OracleLExperiment(L[0], list(L[1:]))
        trace, count = [], []
        (xo, uo), _, co = orc.mpc(p["x0"][b], m, 2, p["X_targ"], p["U_targ"], orc.OracleClock(p["dt"], T, ns), exp, model, p["Q"],
                                  p["R"], p["Qf"], sat=p["sat"], du=p["du"], trace=trace, count=count)
        assert co == 0
        runs.append((xo, uo, trace, count, exp))
    S = len(sample)
    sess = m4q.EnsembleSession(S, n, m, 2, T, ns, p["dt"], p["sat"], p["du"], plant_kind=_lib.PLANT_PROCESS, plant_per_instance=True,
                               target_cols=p["X_targ"].shape[1])
    try:
        sess.load_problem(p["models"], p["x0"][sample], p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"],
                          p["plant_op0"][sample], np.broadcast_to(p["plant_ops"], (S, 1, 2, 2)))
        assert sess.path_detail() == "complex"
        xs_t = np.stack([r[0].T for r in runs])
        us_t = np.stack([r[1].T for r in runs])
        for k in range(ns):
            if k > 0:
                st = {"xs": np.zeros_like(xs_t), "us": np.zeros_like(us_t),
                      "x_guess": np.stack([r[2][k][0].T for r in runs]), "u_guess": np.stack([r[2][k][1].T for r in runs]),
                      "exit_codes": np.zeros(S, dtype=np.int32), "steps_done": np.full(S, k, dtype=np.int32)}
                st["xs"][:, :k + 1] = xs_t[:, :k + 1]
                st["us"][:, :k] = us_t[:, :k]
                sess.restore(st)
            sess.run(k, k + 1)
            got = sess.state()
            assert np.array_equal(sess.download(_lib.F_QP_SOLVES, (S, ns))[:, k], [r[3][k] for r in runs])
            errs = [rel(got["us"][:, k], us_t[:, k]), rel(got["xs"][:, k + 1], xs_t[:, k + 1]),
                    rel(got["x_guess"], np.stack([r[2][k + 1][0].T for r in runs])),
                    rel(got["u_guess"], np.stack([r[2][k + 1][1].T for r in runs]))]
            if not (max(errs[:2]) <= 1e-10 and max(errs[2:]) <= 1e-7):
                sens = np.max([_oracle_step_sensitivity(p, model, runs[i], k, sample[i]) for i in range(S)], axis=0)
                for e, s_k, tol in zip(errs, sens, (1e-10, 1e-10, 1e-7, 1e-7)):
                    assert e <= tol + 10 * s_k, (k, errs, sens.tolist())
            assert np.all(got["exit_codes"] == 0)
    finally:
        sess.close()


def _oracle_step_sensitivity(p, model, run, k, b):
    xo, uo, trace, _, exp = run
    outs = []
    for eps in (0.0, 1e-15, -1e-15, 3e-15):
        tr = []
        st = dict(step=k, xs=xo, us=uo, X_guess=trace[k][0] * (1 + eps), U_guess=trace[k][1])
        (x2, u2), _, _ = orc.mpc(p["x0"][b], 1, 2, p["X_targ"], p["U_targ"], orc.OracleClock(p["dt"], p["horizon"], p["n_steps"]),
                                 exp, model, p["Q"], p["R"], p["Qf"], sat=p["sat"], du=p["du"], start=st, stop=k + 1, trace=tr)
        outs.append((u2[:, k], x2[:, k + 1], tr[-1][0], tr[-1][1]))
    return [max(np.abs(o[i] - outs[0][i]).max() for o in outs[1:]) for i in range(4)]


# ---------------------------------------------------------------- 4. the path trap
def test_process_plant_forces_complex_path():
    """A process problem whose model and data WOULD pass the Hermitian lift (model: the Liouvillian of a 4 x 4 Hermitian
    operator; P0 and the target Hermitian as 4 x 4 matrices; Q, R real) - the same session without the process plant runs on a
    real path.  With M4Q_PLANT_PROCESS it runs on path 0 (V (x) V^* does not keep M Hermitian) and matches the oracle."""
    p = configs.synthesis(1, 1, n_steps=10)
    Hc = np.kron(SZ, np.identity(2)) - np.kron(np.identity(2), SZ.conj())   # 4 x 4 Hermitian
    Hx = np.kron(0.5 * SX, np.identity(2)) - np.kron(np.identity(2), 0.5 * SX.conj())
    from mpc4quantum_amd.vectorize import liouvillian
    models = m4q.discretize_homogeneous([0.1 * liouvillian(Hc), liouvillian(Hx)], p["dt"], 1)[None]
    Ur = np.array([[np.cos(0.3), np.sin(0.3)], [np.sin(0.3), -np.cos(0.3)]], dtype=complex)   # real symmetric unitary
    x0 = np.kron(Ur, Ur.conj()).reshape(1, -1)
    M0 = x0.reshape(4, 4)
    assert np.abs(M0 - M0.conj().T).max() == 0 and np.abs(p["target"].reshape(4, 4) - p["target"].reshape(4, 4).conj().T).max() == 0
    ns, T = p["n_steps"], p["horizon"]
    cols = p["X_targ"].shape[1]
    probe = m4q.EnsembleSession(1, 16, 1, 1, T, ns, p["dt"], p["sat"], p["du"], plant_kind=_lib.PLANT_NONE, target_cols=cols)
    try:
        probe.load_problem(models, x0, p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"])
        assert probe.path() == "real"                               # the data pass the lift ...
    finally:
        probe.close()
    H0 = 0.2 * SZ
    clock = m4q.StepClock(p["dt"], T, ns)
    res = m4q.mpc_batch(x0, models, 1, 1, p["X_targ"], p["U_targ"], clock, H0[None], p["plant_ops"], p["Q"], p["R"], p["Qf"],
                        p["sat"], p["du"], plant_kind=_lib.PLANT_PROCESS)
    assert res["path"] == "complex"                                  # ... and the process plant keeps them off it
    L = process_generators([H0, p["plant_ops"][0, 0]])
    (xo, uo), _, co = orc.mpc(x0[0], 1, 1, p["X_targ"], p["U_targ"], orc.OracleClock(p["dt"], T, ns),
                              orc.OracleLExperiment(L[0], list(L[1:])), orc.OracleDMDc(16, 16, 16, models[0]), p["Q"], p["R"],
                              p["Qf"], sat=p["sat"], du=p["du"])
    assert co == 0 and np.all(res["exit_codes"] == 0)
    assert rel(res["us"][0], uo) <= 1e-9 and rel(res["xs"][0], xo) <= 1e-9        # (controls held by the du band: well determined)
    M = res["xs"][0][:, -1].reshape(4, 4)
    assert np.abs(M - M.conj().T).max() > 1e-3                      # the state did leave the Hermitian matrices


# ---------------------------------------------------------------- 5. exact box-QP mode
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_exact_qp_vs_bvls(order):
    """exact_qp=True on the NOT scenario: the controls of the first MPC steps equal the oracle's BVLS solve of the box QP
    (oracle.exact_quad_program) to 1e-9; an exit code 2 (iteration cap) is a failure here, not an admitted outcome."""
    ns = 6
    p = configs.synthesis(1, order, n_steps=ns)
    exp = m4q.QSynthesis(p["plant_op0"][0], list(p["plant_ops"][0]))
    model = m4q.DMDc(16, 16, p["models"].shape[2] - 16, p["models"][0])
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    (xs, us), _, code = m4q.mpc(p["x0"][0], 1, order, p["X_targ"], p["U_targ"], clock, exp, model, p["Q"], p["R"], p["Qf"],
                                sat=p["sat"], du=p["du"], progress_bar=False, exact_qp=True)
    assert code == 0, "exit code %d (2: the exact solve stopped at its iteration cap)" % code
    L = process_generators([p["plant_op0"][0], p["plant_ops"][0, 0]])
    (xo, uo), _, co = orc.mpc(p["x0"][0], 1, order, p["X_targ"], p["U_targ"], orc.OracleClock(p["dt"], p["horizon"], ns),
                              orc.OracleLExperiment(L[0], list(L[1:])), orc.OracleDMDc(16, 16, p["models"].shape[2] - 16,
                                                                                        p["models"][0]),
                              p["Q"], p["R"], p["Qf"], sat=p["sat"], du=p["du"], qp_mode="exact")
    assert co == 0 and us.shape == uo.shape == (1, ns)
    assert rel(us, uo) <= 1e-9 and rel(xs, xo) <= 1e-9

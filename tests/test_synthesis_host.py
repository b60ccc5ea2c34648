"""Gate synthesis (QSynthesis, M4Q_PLANT_PROCESS) on the host: the helpers against the reference's own outputs
(tests/golden/synthesis.npz, written by tests/golden/make_golden_synthesis.py), the process step against the oracle's generator
plant, and the oracle's closed loop at the new shape (n = 16, one control, orders 1-4) against the reference's mpc.py."""
import os

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from oracle import m4q_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthesis.npz")
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def process_step(P, u, H0, Hs, dt):
    """NumPy process step: vec_r((V (x) V^*) M), V = expm(-i dt (H0 + sum u_k H_k))."""
    from scipy.linalg import expm
    H = H0 + sum(float(uk) * h for uk, h in zip(u, Hs))
    V = expm(-1j * dt * H)
    d = V.shape[0]
    return (np.kron(V, V.conj()) @ np.reshape(P, (d * d, d * d))).reshape(-1)


def process_generators(Hs):
    """L_k (x) I_{d^2} with L_k = -i (H_k (x) I - I (x) H_k^*): the process plant as a generator on vec_r(M)."""
    d = Hs[0].shape[0]
    eye = np.identity(d)
    return [np.kron(-1j * (np.kron(h, eye) - np.kron(eye, h.conj())), np.identity(d * d)) for h in Hs]


def test_lift_proj_match_reference(g):
    for i in range(int(g["lp2_count"])):
        U = g["lp2_%d_U" % i]
        assert np.abs(m4q.QSynthesis.lift(U) - g["lp2_%d_lift" % i]).max() <= 1e-15
        assert np.abs(m4q.QSynthesis.proj(g["lp2_%d_lift" % i]) - g["lp2_%d_proj" % i]).max() <= 1e-15
    assert np.abs(m4q.QSynthesis.lift(g["lp4_U"]) - g["lp4_lift"]).max() <= 1e-15
    assert np.abs(m4q.QSynthesis.proj(g["lp4_lift"]) - g["lp4_proj"]).max() <= 1e-15
    assert np.abs(m4q.QSynthesis.proj(g["lpg_P"]) - g["lpg_proj"]).max() <= 1e-15
    # sigma_x: the first block of U (x) U^* is zero, proj finds the next one; U back up to a global phase
    P = m4q.QSynthesis.lift(SX.reshape(-1))
    assert not np.any(P[:2]) and np.abs(m4q.QSynthesis.lift(m4q.QSynthesis.proj(P)) - P).max() <= 1e-15


def test_qsynthesis_interface():
    exp = m4q.QSynthesis(0.0 * SZ, [0.5 * SX])
    assert exp.plant_kind == _lib.PLANT_PROCESS == 3
    exp.set("options", {"atol": 1e-12})                       # kept and ignored, like QExperiment.set
    with pytest.raises(ValueError, match="c_ops"):
        exp.set("c_ops", [SZ])
    op0, ops = exp.operators()
    assert op0.shape == (2, 2) and ops.shape == (1, 2, 2)
    assert m4q.process_dim(16) == 2 and m4q.process_dim(81) == 3
    with pytest.raises(ValueError):
        m4q.process_dim(9)


def test_process_step_equals_oracle_generator_step():
    rng = np.random.default_rng(5)
    dt = 0.05
    for _ in range(8):
        H0 = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
        H0 = H0 + H0.conj().T
        Hs = [0.5 * SX]
        u = rng.uniform(-1, 1, 1)
        U = np.linalg.qr(rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)))[0]
        for P in (np.kron(U, U.conj()).reshape(-1), rng.standard_normal(16) + 1j * rng.standard_normal(16)):
            L = process_generators([H0] + Hs)
            a = process_step(P, u, H0, Hs, dt)
            b = orc.plant_step_generator(P, u, L[0], L[1:], dt)
            assert np.abs(a - b).max() <= 1e-14


def test_process_step_is_f():
    """QSynthesis.f is the derivative the step integrates: (P(dt) - P(-dt)) / 2 dt -> f."""
    rng = np.random.default_rng(6)
    exp = m4q.QSynthesis(0.3 * SZ, [0.5 * SX])
    P = rng.standard_normal(16) + 1j * rng.standard_normal(16)
    h = 1e-5
    fd = (process_step(P, [0.4], exp.H0, exp.H1_list, h) - process_step(P, [0.4], exp.H0, exp.H1_list, -h)) / (2 * h)
    assert np.abs(fd - exp.f(0.0, P, [0.4])).max() <= 1e-8


def _case(g, name):
    k = "not_%s_" % name
    return {key[len(k):]: g[key] for key in g.files if key.startswith(k)}


@pytest.mark.parametrize("name", ["o1", "o2", "o3", "o4", "o1_exit_mid", "o3_exit_mid", "o1_detuned", "o2_detuned"])
def test_oracle_lqr_loop_matches_reference_mpc_py(g, name):
    """oracle.mpc(qp_mode='lqr') with the process plant written as OracleLExperiment(L_k (x) I_4) reproduces the reference's
    mpc.py around its own lqr.py on the NOT-gate scenario: exit code, shapes, ts_sim, states and controls."""
    c = _case(g, name)
    order = int(c["order"])
    n, m = 16, 1
    Hp = list(c["H_plant"])
    L = process_generators(Hp)
    exp = orc.OracleLExperiment(L[0], L[1:])
    model = orc.OracleDMDc(n, n, c["model"].shape[1] - n, c["model"])
    clock = orc.OracleClock(float(g["not_dt"]), int(g["not_T"]), int(g["not_n_steps"]))
    exit_condition = None
    if bool(c["exit"]):
        pf, Q, thr = g["not_pf"], g["not_Q"], float(c["exit_thr"])
        exit_condition = lambda p2, p1, u1: ((p1 - pf).conj() @ Q @ (p1 - pf)).real < thr       # noqa: E731
    (xs, us), _, code = orc.mpc(g["not_p0"], m, order, g["not_X_targ"], g["not_U_targ"], clock, exp, model, g["not_Q"],
                                g["not_R"], g["not_Qf"], sat=float(g["not_sat"]), du=float(g["not_du"]), qp_mode="lqr",
                                exit_condition=exit_condition)
    assert code == int(c["exit_code"])
    assert xs.shape == c["xs"].shape and np.array_equal(clock.ts_sim, c["ts_sim"])
    assert_matches_reference(xs, us, c)


def assert_matches_reference(xs, us, c, tol=1e-9):
    """States and controls step by step within tol plus 100 times what the REFERENCE's own run moves when P0 is scaled by
    1 +- 1e-14 (env_*, running maximum): at order 1 the loop chatters between the bounds and an interior control decides a later
    switch (env_us reaches 7e-4 by step 36)."""
    env_x, env_u = c["env_xs"], c["env_us"]
    assert np.all(np.abs(xs - c["xs"]).max(axis=0) <= tol + 100 * env_x), np.abs(xs - c["xs"]).max(axis=0)
    if bool(c["us_is_none"]):
        assert us is None
    else:
        assert us.shape == c["us"].shape
        assert np.all(np.abs(us - c["us"]).max(axis=0) <= tol + 100 * env_u), np.abs(us - c["us"]).max(axis=0)


def involution(P):
    """J: P[(a,b),(k,l)] -> conj(P[(b,a),(l,k)]), an antiunitary involution on process vectors.  Lifted unitaries U (x) U^* are
    fixed by it, and L (x) I commutes with it: the closed loop never leaves its fixed (real) subspace."""
    d = int(round(P.shape[0] ** 0.25))
    t = np.reshape(P, (d, d, d, d) + P.shape[1:])
    return np.conj(np.swapaxes(np.swapaxes(t, 0, 1), 2, 3)).reshape(P.shape)


def test_quad_program_is_kkt_on_a_process_qp():
    """The oracle's Riccati QP (real part of the complex gain) equals the dense real KKT solve on a process QP whose data lie in
    the fixed subspace of the involution J (states, targets, the guess the model is linearised along): there the complex
    recursion is a real one in disguise and the real part of its gain is the real-control optimum, as for density matrices.
    A guess off that subspace makes B_t leave it, and then it is not (the check is sharp)."""
    p = configs.synthesis(1, 2)
    n, m, T = 16, 1, 6
    rng = np.random.default_rng(9)
    assert np.abs(involution(p["x0"][0]) - p["x0"][0]).max() == 0 and np.abs(involution(p["target"]) - p["target"]).max() == 0
    wm = orc.OracleWrapModel(p["models"][0][:, :n], p["models"][0][:, n:], m, 2)
    Z = 1e-2 * (rng.standard_normal((n, T + 1)) + 1j * rng.standard_normal((n, T + 1)))
    Ug = 0.3 * rng.standard_normal((m, T))
    X_bm = p["X_targ"][:, :T + 1]
    U_bm = p["U_targ"][:, :T]
    Q_ls = [p["Q"]] * T + [p["Qf"]]
    R_ls = [p["R"]] * T
    x0 = p["x0"][0]
    errs = []
    for guess in (0.5 * (Z + involution(Z)), Z):
        Xg = np.tile(x0.reshape(-1, 1), (1, T + 1)) + guess
        A_ls, B_ls, D_ls = wm.get_model_along_traj(Xg, Ug, np.arange(T) * p["dt"])
        X1, U1, _, _ = orc.quad_program(x0, X_bm, U_bm, Q_ls, R_ls, A_ls, B_ls, D_ls, None, 1e6, None)
        X2, U2 = orc.kkt_quad_program(x0, X_bm, U_bm, Q_ls, R_ls, A_ls, B_ls, D_ls)
        assert np.abs(U2).max() > 1.0
        errs.append((rel(U1, U2), rel(X1, X2)))
    assert errs[0][0] <= 1e-9 and errs[0][1] <= 1e-9
    assert errs[1][0] > 1e-6


def test_synthesis_config():
    p = configs.synthesis(8, 3, detuning_spread=0.2)
    assert p["dim_x"] == 16 and p["dim_u"] == 1 and p["plant_kind"] == _lib.PLANT_PROCESS
    assert p["models"].shape == (1, 16, 16 * 4) and p["plant_op0"].shape == (8, 2, 2) and p["plant_ops"].shape == (1, 1, 2, 2)
    assert p["X_targ"].shape[1] >= p["n_steps"] + p["horizon"] - 1
    assert np.allclose(p["plant_op0"], 0.5 * p["detunings"][:, None, None] * SZ)
    ref = orc.discretize_homogeneous(list(p["generators"]), p["dt"], 3)
    assert np.abs(p["models"][0] - ref).max() <= 1e-15


def test_process_shapes_supported():
    assert _lib.PLANT_PROCESS == 3
    for k in (1, 2, 3, 4):
        assert _lib.supported(16, 1, k)

"""Every compiled kernel variant against the oracle, cell by cell (-m gpu).

The cells come from tests/kernel_variants.py, which mirrors the rules that decide which mpc_kernel instances each shape's object
holds (m4q_kernels.hip pick_kernel / pick_plant, build.py's generator-plant library); tests/test_kernel_variants_host.py pins those
mirrors to the sources.  A closed-loop cell is shape x arithmetic path x exact flag x plant kind: its session must report the
cell's path (a host-side fallback cannot pass as coverage) and every MPC step is teacher-forced from the oracle's run of the same
scenario.  Fixed bounds, no sensitivity clause: the scenarios are conditioned so that the oracle itself moves by at most 3e-12 on
a step's outputs and 6e-12 on the guesses it leaves behind when the guess the step starts from is perturbed by 1e-15 (measured
on every shape, both plants, both solves).  The entry-point cells hold linearize, quad_program, discretize and plant_step of each
shape to the oracle at the suite's tolerances."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from oracle import m4q_oracle as orc
from tests import kernel_variants as kv
from tests import strong_drive_cases as sd

pytestmark = pytest.mark.gpu

LOOP_CELLS = kv.closed_loop_cells()
ENTRY_CELLS = kv.entry_point_cells()


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


# ---------------------------------------------------------------- closed-loop cells
_ORACLE = {}


def _plant_ops(p, plant):
    """(op0, ops, generator_plant) of the oracle's plant for a cell: the scenario's Hamiltonians, or its generators (generator
    plant; the process plant as generators on P; PLANT_NONE cells take the generator plant's trajectory - the host supplies it)."""
    if plant == kv.HAMILTONIAN:
        return p["plant_op0"], p["plant_ops"], False
    return p["gen_op0"], p["gen_ops"], True


def _scenario(cell):
    return kv.process_scenario(cell.nu, cell.order) if cell.plant == kv.PROCESS else kv.scenario(cell.nx, cell.nu, cell.order)


def _oracle(cell, exact):
    """The oracle's run of the cell's scenario (cached: every path of one shape and plant shares it)."""
    oracle_plant = kv.HAMILTONIAN if cell.plant == kv.HAMILTONIAN else kv.PROCESS if cell.plant == kv.PROCESS else kv.GENERATOR
    key = (cell.nx, cell.nu, cell.order, oracle_plant, exact)
    if key not in _ORACLE:
        p = _scenario(cell)
        op0, ops, gen = _plant_ops(p, oracle_plant)
        trace = []
        xs, us, codes, solves = orc.mpc_batch(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], p["dt"],
                                              p["horizon"], p["n_steps"], op0, list(ops[0]), p["Q"], p["R"], p["Qf"], p["sat"],
                                              p["du"], qp_mode="exact" if exact else "qp", trace=trace, generator_plant=gen)
        _ORACLE[key] = (p, np.swapaxes(xs, 1, 2), np.swapaxes(us, 1, 2), codes, solves, trace)   # time-major
    return _ORACLE[key]


def _open(cell, p, model_per_instance=None, target_per_instance=False, plant_per_instance=None):
    """A session of the cell's kernel on scenario p (model_per_instance: default, whether p holds one model per member;
    plant_per_instance: default, the process cells - detuned members, one d x d Hamiltonian each; target_per_instance: X_targ and
    U_targ of p carry a leading member axis)."""
    B, n, m = p["batch"], p["dim_x"], p["dim_u"]
    per_plant = cell.plant == kv.PROCESS if plant_per_instance is None else plant_per_instance
    op0, ops, _ = _plant_ops(p, kv.HAMILTONIAN if cell.plant == kv.PROCESS else cell.plant)
    if model_per_instance is None:
        model_per_instance = p["models"].shape[0] > 1
    sess = m4q.EnsembleSession(B, n, m, p["order"], p["horizon"], p["n_steps"], p["dt"], p["sat"], p["du"],
                               plant_kind=kv.PLANT_CODE[cell.plant], model_per_instance=model_per_instance,
                               plant_per_instance=per_plant, target_per_instance=target_per_instance,
                               target_cols=p["n_steps"] + p["horizon"] + 1,
                               force_complex=cell.path == kv.COMPLEX, traceless=cell.path != kv.REAL, tile=cell.path == kv.TILE,
                               shared_generators=None if cell.path == kv.SG else False, exact_qp=cell.exact)
    try:
        if cell.path == kv.SG:
            sess.build_models(p["dt"], p["generators"], p["scales"])
        if per_plant and cell.plant != kv.NONE:
            op0 = np.broadcast_to(op0, (B,) + op0.shape[1:])
            ops = np.broadcast_to(ops, (B,) + ops.shape[1:])
        sess.load_problem(None if cell.path == kv.SG else p["models"], p["x0"], p["X_targ"], p["U_targ"], p["Q"], p["R"], p["Qf"],
                          None if cell.plant == kv.NONE else op0, None if cell.plant == kv.NONE else ops)
    except Exception:
        sess.close()
        raise
    return sess


def _teacher_forced(cell, run, path=None, **open_kw):
    """One kernel instance on the oracle's run (p, xs_t, us_t, codes, solves, trace) of a scenario: every MPC step started from the
    oracle's state (states, controls, SQP guesses; PLANT_NONE: the state through put_state, as the host-driven loop hands it over).
    The session (opened with open_kw) reports `path` (default: the cell's) before the first step and after the last; exit codes 0
    and identical QP-solve counts at every step.  Clipped solve: us[k] and xs[k+1] to 1e-10 relative, the SQP guesses left behind to
    1e-7.  Exact solve: us[k] within 1e-9 of the bound, xs[k+1] within 1e-9.  Returns (the applied controls, the number of control
    and guess entries seen at the bound, the worst error over its bound)."""
    p, xs_t, us_t, codes, solves, trace = run
    assert np.all(codes == 0)
    B, ns, sat = p["batch"], p["n_steps"], p["sat"]
    path = cell.path if path is None else path
    worst = 0.0
    sess = _open(cell, p, **open_kw)
    try:
        assert sess.path_detail() == path
        at_bound = 0
        us_got = np.zeros_like(us_t)
        for k in range(ns):
            if k > 0:
                st = {"xs": np.zeros_like(xs_t), "us": np.zeros_like(us_t),
                      "x_guess": np.stack([trace[b][k][0].T for b in range(B)]),
                      "u_guess": np.stack([trace[b][k][1].T for b in range(B)]),
                      "exit_codes": np.zeros(B, dtype=np.int32), "steps_done": np.full(B, k, dtype=np.int32)}
                st["xs"][:, :k + 1] = xs_t[:, :k + 1]
                st["us"][:, :k] = us_t[:, :k]
                if cell.plant == kv.NONE:
                    st["xs"][:, k] = 0
                sess.restore(st)
            if cell.plant == kv.NONE:
                sess.put_state(k, xs_t[:, k])
            sess.run(k, k + 1)
            got = sess.state()
            assert np.all(got["exit_codes"] == 0) and np.all(got["steps_done"] == k + 1), k
            assert np.array_equal(sess.download(_lib.F_QP_SOLVES, (B, ns))[:, k], solves[:, k]), k
            us_got[:, k] = got["us"][:, k]
            if cell.exact:
                eu = np.abs(got["us"][:, k] - us_t[:, k]).max() / sat
                ex = np.abs(got["xs"][:, k + 1] - xs_t[:, k + 1]).max() if cell.plant != kv.NONE else 0.0
                worst = max(worst, eu / 1e-9, ex / 1e-9)
                assert eu <= 1e-9 and ex <= 1e-9, (k, eu, ex)
                at_bound += int((np.abs(got["us"][:, k]) >= sat * (1 - 1e-9)).sum() + (np.abs(got["u_guess"]) >= sat * (1 - 1e-9)).sum())
            else:
                errs = [rel(got["us"][:, k], us_t[:, k]),
                        rel(got["xs"][:, k + 1], xs_t[:, k + 1]) if cell.plant != kv.NONE else 0.0,
                        rel(got["x_guess"], np.stack([trace[b][k + 1][0].T for b in range(B)])),
                        rel(got["u_guess"], np.stack([trace[b][k + 1][1].T for b in range(B)]))]
                worst = max(worst, max(errs[:2]) / 1e-10, max(errs[2:]) / 1e-7)
                assert max(errs[:2]) <= 1e-10 and max(errs[2:]) <= 1e-7, (k, errs)
                at_bound += int((np.abs(got["u_guess"]) >= sat * (1 - 1e-9)).sum())
        assert sess.path_detail() == path                      # (the line-search weights are known after the first run)
    finally:
        sess.close()
    assert np.abs(us_got).max() <= sat * (1 + 1e-15)
    return us_got, at_bound, worst


@pytest.mark.parametrize("cell", LOOP_CELLS, ids=kv.cell_id)
def test_closed_loop_cell_teacher_forced(cell):
    """One kernel instance: every MPC step started from the oracle's state (states, controls, SQP guesses; PLANT_NONE: the state
    through put_state, as the host-driven loop hands it over).  Clipped solve: QP-solve counts identical, us[k] and xs[k+1] to
    1e-10 relative, the SQP guesses left behind to 1e-7.  Exact solve: counts identical, us[k] within 1e-9 of the bound, xs[k+1]
    within 1e-9, some control at the bound, and the controls differ from the clipped loop's.  Exit codes 0 throughout.  With no
    plant the next state is the host's: us[k], the guesses and the counts are the kernel's outputs."""
    p = _oracle(cell, cell.exact)[0]
    sat = p["sat"]
    us_got, at_bound, _ = _teacher_forced(cell, _oracle(cell, cell.exact))
    assert at_bound > 0, "no control at the bound: the scenario does not exercise the box"
    if cell.exact:
        clip = _oracle(cell, False)[2]
        assert np.abs(us_got - clip).max() > 1e-3 * sat         # the bounds matter: the clipped loop lands elsewhere


# ---------------------------------------------------------------- entry-point cells
def _cells(kind):
    return [c for c in ENTRY_CELLS if c.kind == kind]


def _density_states(rng, d, B):
    out = []
    for _ in range(B):
        M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        r = M @ M.conj().T
        out.append((r / np.trace(r).real).reshape(-1))
    return np.stack(out)


@pytest.mark.parametrize("cell", _cells("linearize"), ids=kv.cell_id)
def test_linearize_cell(cell):
    """m4q_linearize_batch at the shape, B = 7, shared and per-instance models, against OracleWrapModel.get_model_along_traj
    (1e-13; Delta 1e-12).  Controls of order one, so every power of the library (u^3, u^4 at orders 3-4) carries weight."""
    Bn, T = 7, 5
    p = kv.scenario(cell.nx, cell.nu, cell.order, batch=Bn)
    n, m = cell.nx, cell.nu
    rng = np.random.default_rng(7 + n + 10 * m + 100 * cell.order)
    X = rng.standard_normal((Bn, T, n)) + 1j * rng.standard_normal((Bn, T, n))
    U = rng.uniform(-1.2, 1.2, (Bn, T, m))
    models = p["models"]
    wm = m4q.WrapModel(models[0][:, :n], models[0][:, n:], m, cell.order)
    A_s, B_s, D_s = wm.linearize_batch(X, U)
    A = np.empty((Bn, T, n, n), dtype=complex)
    Bm = np.empty((Bn, T, n, m), dtype=complex)
    D = np.empty((Bn, T, n), dtype=complex)
    L = _lib.lib()
    _lib.check(L.m4q_linearize_batch(Bn, n, m, cell.order, T, _lib.cbuf(models)[1], 1, _lib.cbuf(X)[1], _lib.rbuf(U)[1],
                                     A.ctypes.data_as(_lib._dp), Bm.ctypes.data_as(_lib._dp), D.ctypes.data_as(_lib._dp)))
    for b in range(Bn):
        for mod, (Ag, Bg, Dg) in ((models[0], (A_s, B_s, D_s)), (models[b], (A, Bm, D))):
            wo = orc.OracleWrapModel(mod[:, :n], mod[:, n:], m, cell.order)
            Ao, Bo, Do = wo.get_model_along_traj(X[b].T, U[b].T, np.arange(T))
            assert rel(Ag[b], np.stack(Ao)) <= 1e-13
            assert rel(Bg[b], np.stack(Bo)) <= 1e-13
            assert rel(Dg[b], np.stack(Do)[:, :, 0]) <= 1e-12
    assert rel(A, A_s) > 1e-6                                   # the members' models do differ


def _random_ltv(rng, n, m, T, Bn):
    A = np.eye(n) + 0.3 * (rng.standard_normal((Bn, T, n, n)) + 1j * rng.standard_normal((Bn, T, n, n))) / np.sqrt(n)
    Bm = 0.5 * (rng.standard_normal((Bn, T, n, m)) + 1j * rng.standard_normal((Bn, T, n, m)))
    D = 0.05 * (rng.standard_normal((Bn, T, n)) + 1j * rng.standard_normal((Bn, T, n)))
    x0 = rng.standard_normal((Bn, n)) + 1j * rng.standard_normal((Bn, n))
    Xb = 0.5 * (rng.standard_normal((Bn, T + 1, n)) + 1j * rng.standard_normal((Bn, T + 1, n)))
    Ub = 0.2 * rng.standard_normal((Bn, T, m))
    Qs, Rs = [], []
    for _ in range(T + 1):
        M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        Qs.append(M @ M.conj().T / n)
    for _ in range(T):
        M = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
        Rs.append(M @ M.conj().T / m + 0.5 * np.eye(m))
    return A, Bm, D, x0, Xb, Ub, np.stack(Qs), np.stack(Rs)


def _scenario_qp(nx, nu, Bn, T, seed):
    """The scenario's models linearised along a perturbed guess (Hermiticity preserving: the box QP's real-control optimum is what
    the Riccati factorisation finds), its own control reference and bound."""
    rng = np.random.default_rng(seed)
    order = min(o for x, u, o, po in kv.shapes() if (x, u) == (nx, nu) and not po)
    p = kv.scenario(nx, nu, order, batch=Bn, horizon=T)
    n, m = nx, nu
    A, Bm, D = [], [], []
    for b in range(Bn):
        mod = p["models"][b]
        wm = orc.OracleWrapModel(mod[:, :n], mod[:, n:], m, order)
        xg = np.tile(p["x0"][b][:, None], (1, T + 1))
        ug = 0.3 * p["sat"] * rng.uniform(-1, 1, (m, T))
        Ao, Bo, Do = wm.get_model_along_traj(xg, ug, np.arange(T))
        A.append(np.stack(Ao)); Bm.append(np.stack(Bo)); D.append(np.stack(Do).reshape(T, n))
    Qs = np.stack([p["Q"]] * T + [p["Qf"]]).astype(complex)
    Rs = np.stack([p["R"]] * T).astype(complex)
    return (p["x0"], p["X_targ"][:, :T + 1].T[None], np.real(p["U_targ"][:, :T]).T[None], Qs, Rs, np.stack(A), np.stack(Bm),
            np.stack(D), 0.5 * p["sat"])


@pytest.mark.parametrize("cell", _cells("qp"), ids=kv.cell_id)
def test_quad_program_cell(cell):
    """m4q_quad_program_batch at (n, m) in one mode against the oracle, 1e-9.  qp / du band / REF_LQR: dense complex LTV problems
    with time-varying costs, bounds inactive and active.  exact: the scenario's linearised QP against BVLS, bounds active and
    mattering (as test_exact_box_qp_vs_bvls_oracle)."""
    n, m = cell.nx, cell.nu
    rng = np.random.default_rng(200 + n + 10 * m)
    T, Bn = 7, 6
    if cell.mode == "exact":
        x0, Xb, Ub, Qs, Rs, A, Bm, D, sat = _scenario_qp(n, m, 5, T, 300 + n + 10 * m)
        X, U, cost, _ = m4q.quad_program_batch(x0, Xb, Ub, Qs, Rs, A, Bm, D, None, sat, None, exact=True)
        Xc, Uc, costc, _ = m4q.quad_program_batch(x0, Xb, Ub, Qs, Rs, A, Bm, D, None, sat, None)
        assert np.abs(U).max() <= sat and np.all(cost <= costc * (1 + 1e-14))
        active = 0
        for b in range(len(x0)):
            Xe, Ue, ce = orc.exact_quad_program(x0[b], Xb[0].T, Ub[0].T, list(Qs), list(Rs), list(A[b]), list(Bm[b]), list(D[b]),
                                                None, sat, None)
            assert np.abs(U[b].T - Ue).max() <= 1e-9 * min(sat, 1.0)
            assert rel(X[b].T, Xe) <= 1e-9
            assert abs(cost[b] - ce) <= 1e-11 * max(1.0, abs(ce))
            active += int((np.abs(Ue) >= sat * (1 - 1e-12)).sum())
        assert active > 0 and np.abs(U - Uc).max() > 1e-4 * sat
        return
    A, Bm, D, x0, Xb, Ub, Qs, Rs = _random_ltv(rng, n, m, T, Bn)
    uprev = 0.1 * rng.standard_normal((Bn, m))
    cases = {"qp": ((1e3, None), (0.3, None)), "du_band": ((0.6, 0.2), (1e3, 0.05)), "ref_lqr": ((1e3, None), (0.3, None))}[cell.mode]
    for sat, du in cases:
        if cell.mode == "ref_lqr":
            X, U, cost, gains = m4q.quad_program_batch(x0, Xb, Ub, Qs, Rs, A, Bm, None, None, sat, None, flags=_lib.QP_REF_LQR)
        else:
            X, U, cost, gains = m4q.quad_program_batch(x0, Xb, Ub, Qs, Rs, A, Bm, D, uprev if du else None, sat, du)
        for b in range(Bn):
            if cell.mode == "ref_lqr":
                Xo, Uo, co, go = orc.lqr_quad_program(x0[b], Xb[b].T, Ub[b].T, list(Qs), list(Rs), list(A[b]), list(Bm[b]), None,
                                                      sat, None)
            else:
                Xo, Uo, co, go = orc.quad_program(x0[b], Xb[b].T, Ub[b].T, list(Qs), list(Rs), list(A[b]), list(Bm[b]), list(D[b]),
                                                  uprev[b] if du else None, sat, du)
            assert rel(gains[b], np.stack([gk.T for gk in go])) <= 1e-9
            assert rel(X[b].T, Xo) <= 1e-9
            assert rel(U[b].T, Uo) <= 1e-9
            assert abs(cost[b] - co) <= 1e-9 * max(1.0, abs(co))
        if sat < 1:
            assert np.abs(U).max() >= sat * (1 - 1e-15)       # the bound is active in this case
        if du:
            assert np.all(np.abs(U[:, 0, :] - uprev) <= du + 1e-15)
            assert np.abs(U[:, 0, :] - uprev).max() >= du * (1 - 1e-12)    # ... and the band is too
        assert np.abs(U).max() <= sat + 1e-15


@pytest.mark.parametrize("cell", _cells("discretize"), ids=kv.cell_id)
def test_discretize_cell(cell):
    """m4q_discretize_batch at the shape against orc.discretize_homogeneous (1e-13): shared generators, per-member generators,
    shared generators with per-member scales; general complex generators (a Liouvillian plus a perturbation where n = d^2)."""
    rng = np.random.default_rng(50 + cell.nx + 10 * cell.nu + 100 * cell.order)
    n, m, d = cell.nx, cell.nu, kv.dd(cell.nx)
    Bn, dt = 7, 0.3

    def gen():
        G = 0.1 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        if kv.square(n):
            H = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
            G = G + m4q.liouvillian(H + H.conj().T)
        return G
    Ls = [gen() for _ in range(m + 1)]
    shared = m4q.discretize_homogeneous_batch(Ls, dt, cell.order)
    assert shared.shape[0] == 1 and rel(shared[0], orc.discretize_homogeneous(Ls, dt, cell.order)) <= 1e-13
    per = [np.stack([L * (1 + 0.1 * b) + 0.01 * b * gen() for b in range(Bn)]) for L in Ls]
    out = m4q.discretize_homogeneous_batch(per, dt, cell.order)
    scales = 1 + 0.1 * rng.standard_normal((Bn, m + 1))
    out_s = m4q.discretize_homogeneous_batch(Ls, dt, cell.order, scales=scales)
    for b in range(Bn):
        assert rel(out[b], orc.discretize_homogeneous([L[b] for L in per], dt, cell.order)) <= 1e-13
        assert rel(out_s[b], orc.discretize_homogeneous([scales[b, k] * Ls[k] for k in range(m + 1)], dt, cell.order)) <= 1e-13


# the large controls of test_plant_step_cell where 40 leaves a member at s = 0 or all five at one s: the lowest of 80, 160, .. at
# which every member squares and s differs within the five (tests/strong_drive_cases.py: squarings mirrors expm_cols' rule)
LARGE_CONTROLS = {(4, 1, kv.HAMILTONIAN): 80.0, (4, 1, kv.GENERATOR): 2560.0, (4, 2, kv.HAMILTONIAN): 80.0, (4, 2, kv.GENERATOR): 80.0,
                  (16, 1, kv.GENERATOR): 80.0, (16, 2, kv.HAMILTONIAN): 80.0}


@pytest.mark.parametrize("cell", _cells("plant"), ids=kv.cell_id)
def test_plant_step_cell(cell):
    """m4q_plant_step_batch at (n, m) against orc.plant_step (Hamiltonian, 1e-12) / plant_step_generator (Lindbladian, 1e-11), B = 5
    with per-member operators, and one case with large controls that forces scaling and squaring: s >= 1 for every member and
    differing within the five, asserted."""
    rng = np.random.default_rng(60 + cell.nx + 10 * cell.nu)
    n, m, d = cell.nx, cell.nu, kv.dd(cell.nx)
    Bn = 5

    def herm():
        M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        return 0.5 * (M + M.conj().T)
    x = _density_states(rng, d, Bn)
    large = LARGE_CONTROLS.get((n, m, cell.mode), 40.0)

    def squares(exponents):
        s = [sd.squarings(sd.norm1(Z)) for Z in exponents]
        print("%s at controls of %g: s = %s" % (kv.cell_id(cell), large, s))
        assert min(s) >= 1 and len(set(s)) > 1
    if cell.mode == kv.HAMILTONIAN:
        H0 = np.stack([herm() for _ in range(Bn)])
        Hk = np.stack([[herm() for _ in range(m)] for _ in range(Bn)])
        for dt, scale in ((0.25, 1.0), (0.25, large)):
            u = scale * rng.uniform(-1, 1, (Bn, m))
            if scale == large:
                squares(-1j * dt * (H0 + np.einsum('bk,bkij->bij', u, Hk)))
            out = m4q.plant_step_batch(x, u, H0, Hk, dt)
            for b in range(Bn):
                assert rel(out[b], orc.plant_step(x[b], u[b], H0[b], list(Hk[b]), dt)) <= 1e-12
            tr = out.reshape(Bn, d, d).trace(axis1=1, axis2=2)
            assert np.abs(tr - 1).max() < 1e-12
        return
    a = np.diag(np.sqrt(np.arange(1, d)), 1).astype(complex)
    L0 = np.stack([m4q.liouvillian(herm()) + 0.3 * kv.lindblad(a) for _ in range(Bn)])
    Lk = np.stack([[m4q.liouvillian(herm()) for _ in range(m)] for _ in range(Bn)])
    for dt, scale in ((0.1, 1.0), (2.5, 1.0), (0.25, large)):
        u = scale * rng.uniform(-1, 1, (Bn, m))
        if scale == large:
            squares(np.swapaxes(dt * (L0 + np.einsum('bk,bkij->bij', u, Lk)), 1, 2))         # (a lane owns a row of L: expm of L^T)
        out = m4q.plant_step_batch(x, u, L0, Lk, dt, _lib.PLANT_GENERATOR)
        for b in range(Bn):
            assert rel(out[b], orc.plant_step_generator(x[b], u[b], L0[b], list(Lk[b]), dt)) <= 1e-11


# ---------------------------------------------------------------- build_models input shapes
def test_build_models_rejects_bad_shapes_on_a_session():
    """EnsembleSession.build_models refuses generators and scales of any other shape than the C side reads, before the call; the
    accepted forms still build (per-member models, checked against the host expansion)."""
    p = kv.scenario(16, 3, 1)
    B, m = p["batch"], p["dim_u"]
    sess = m4q.EnsembleSession(B, 16, m, 1, p["horizon"], p["n_steps"], p["dt"], p["sat"], p["du"], model_per_instance=True,
                               target_cols=p["n_steps"] + p["horizon"] + 1)
    try:
        g = p["generators"]
        for gens, scales in ((g, p["scales"][0]), (g, p["scales"][:, 0]), (g, p["scales"][:-1]), (np.stack([g] * (B - 1)), None),
                             (g[:-1], p["scales"]), (g[None, None], None)):
            with pytest.raises(ValueError):
                sess.build_models(p["dt"], gens, scales)
        for gens in (g, g[None], np.stack([g] * B)):
            sess.build_models(p["dt"], gens, p["scales"])
            assert rel(sess.download(_lib.F_MODELS, p["models"].shape), p["models"]) <= 1e-14
    finally:
        sess.close()

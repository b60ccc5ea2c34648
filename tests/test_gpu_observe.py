"""Observed plants on the device (-m gpu): the lift kernel against its definition, the residuals of device-resident runs, the
crosstalk run against the oracle, every run against a loop that does the per-step host work (launch, plant_step_batch, NumPy lift,
put_state), the invariances of run_observed, a member that ends early, and mpc() as a drop-in.

Bounds.  Partial trace: two-term sums, bit for bit.  Qubit block: 1e-14 max(1, |x|) - about a dozen roundings of 1.1e-16 (four
squared moduli, the determinant, two square roots, the division) with a factor of eight left.  Plant step: 1e-10 max(1, |z|), the
project's plant bound.  Free-running runs against the host loop: 100 times what the HOST loop itself moves when z0 is scaled by
1 +- 1e-15 (the envelope rule) - measured on the host loop, never on the code under test."""
import functools

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, observe as ob
from mpc4quantum_amd.configs import I2, SX, SY, SZ, rx
from mpc4quantum_amd.mpc import open_session
from mpc4quantum_amd.session import EnsembleSession
from oracle import m4q_oracle as orc

pytestmark = pytest.mark.gpu

PT, QB = ob.OBSERVE_PARTIAL_TRACE, ob.OBSERVE_QUBIT_BLOCK
LIFT_TOL = 1e-14
PLANT_TOL = 1e-10


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def lift_error(kind, x, z):
    """0.0 for a bit-identical partial trace (inf otherwise); the qubit block's error in units of max(1, |x|)."""
    want = ob.observe_reference(kind, z)
    if kind == PT:
        return 0.0 if np.array_equal(x, want) else np.inf
    return float(np.abs(x - want).max() / max(1.0, np.abs(want).max()))


# ---------------------------------------------------------------- lift parity
def _density(rng, d, count):
    a = rng.standard_normal((count, d, d)) + 1j * rng.standard_normal((count, d, d))
    rho = a @ np.conj(np.swapaxes(a, 1, 2))
    return rho / np.trace(rho, axis1=1, axis2=2)[:, None, None]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("kind", [PT, QB])
def test_lift_parity(kind, B):
    """B = 5: one full quad plus a tail row."""
    rng = np.random.default_rng(100 * kind + B)
    n_p, n, d = ob.observe_dims(kind)
    z = _density(rng, d, B).reshape(B, n_p)
    if B > 1:
        z[1] = rng.standard_normal(n_p) + 1j * rng.standard_normal(n_p)          # not a state at all
        if kind == QB:
            v = rng.standard_normal(2) + 1j * rng.standard_normal(2)
            z[2] = 0
            z[2].reshape(3, 3)[:2, :2] = np.outer(v, v.conj())                    # a rank-1 block
            z[3].reshape(3, 3)[:2, :2] *= 1e-8                                    # nearly everything leaked
    x = ob.observe_batch(kind, z)
    err = lift_error(kind, x, z)
    print("lift parity kind %d B %d: max error %.3e" % (kind, B, err))
    assert x.shape == (B, n)
    assert err <= (0.0 if kind == PT else LIFT_TOL)


def test_lift_of_a_zero_block_is_nan():
    z = np.zeros((2, 9), dtype=complex)
    z[:, 8] = 1.0
    z[1, :] = _density(np.random.default_rng(5), 3, 1).reshape(9)
    x = ob.observe_batch(QB, z)
    assert np.all(np.isnan(x[0])) and np.all(np.isfinite(x[1]))


# ---------------------------------------------------------------- scenarios
def crosstalk_case():
    """The scenario of test_mpc_crosstalk_model_on_reduced_states (the reference's tests/test_mpc4quantum.py:281-397), with the
    crosstalk strength per member through op0."""
    cts = np.array([0.0, 0.05, 0.1, 0.2, 0.4])
    dt, T, ns = 0.5, 8, 6
    L1 = [m4q.liouvillian(0 * SX), m4q.liouvillian(SX)]
    L2 = [m4q.liouvillian(0 * SY), m4q.liouvillian(SY)]
    zz = np.zeros((4, 4))
    A_cts = [np.block([[L1[0], zz], [zz, L2[0]]]), np.block([[L1[1], zz], [zz, zz]]), np.block([[zz, zz], [zz, L2[1]]])]
    sat = 2 * np.pi * 0.1
    r1, r2 = rx(1e-2), rx(-1e-2)
    p0, p1 = np.diag([1.0, 0]).astype(complex), np.diag([0, 1.0]).astype(complex)
    rho0 = np.kron(r1 @ p0 @ r1.conj().T, r2 @ p0 @ r2.conj().T)
    target = np.hstack([p1.flatten(), p1.flatten()])
    return dict(kind=PT, n=8, m=2, dt=dt, T=T, ns=ns, model=m4q.discretize_homogeneous(A_cts, dt, 1),
                z0=np.tile(rho0.reshape(1, 16), (len(cts), 1)), op0=np.stack([0.5 * ct * np.kron(SZ, SZ) for ct in cts]),
                ops=np.stack([0.5 * np.kron(SX, I2), 0.5 * np.kron(I2, SY)]), X_bm=np.tile(target[:, None], (1, ns + T + 1)),
                U_bm=np.zeros((2, ns + T)), Q=np.diag([1.0, 0, 0, 1, 1, 0, 0, 1]), R=1e-2 / sat ** 2 * np.eye(2), sat=sat, du=0.5 * sat)


def leaky_case(m):
    """A transmon whose third level the model does not see, in the frame rotating at the qubit frequency: the plant has the
    anharmonicity on |2><2| (per member) and the ladder drives, the model the two-level Liouvillians.  m = 1: H_X alone."""
    alphas = np.array([-2.0, -1.5, -1.0, -3.0, -2.5])
    dt, T, ns = 0.25, 6, 5
    a = np.diag([1.0, np.sqrt(2.0)], 1).astype(complex)
    hx, hy = 0.5 * (a + a.conj().T), 0.5j * (a.conj().T - a)
    plant_ops = np.stack([hx, hy][:m])
    gens = [m4q.liouvillian(0 * SX)] + [m4q.liouvillian(h) for h in (0.5 * SX, 0.5 * SY)[:m]]
    sat = 2 * np.pi * 0.2
    from scipy.linalg import expm
    U0 = expm(-0.1j * hx)
    rho0 = 0.97 * (U0 @ np.diag([1.0, 0, 0]) @ U0.conj().T) + 0.01 * np.eye(3)
    p1 = np.diag([0, 1.0]).astype(complex).flatten()
    return dict(kind=QB, n=4, m=m, dt=dt, T=T, ns=ns, model=m4q.discretize_homogeneous(gens, dt, 1),
                z0=np.tile(rho0.reshape(1, 9), (len(alphas), 1)), op0=np.stack([np.diag([0, 0, al]).astype(complex) for al in alphas]),
                ops=plant_ops, X_bm=np.tile(p1[:, None], (1, ns + T + 1)), U_bm=np.zeros((m, ns + T)), Q=np.eye(4),
                R=1e-2 / sat ** 2 * np.eye(m), sat=sat, du=0.5 * sat)


CASES = {
    "crosstalk": (crosstalk_case, (), {}),
    "crosstalk-exact": (crosstalk_case, (), dict(exact_qp=True)),
    "leaky-2": (leaky_case, (2,), {}),
    "leaky-2-complex": (leaky_case, (2,), dict(force_complex=True)),
    "leaky-2-exact": (leaky_case, (2,), dict(exact_qp=True)),
    "leaky-1": (leaky_case, (1,), {}),
    "leaky-1-complex": (leaky_case, (1,), dict(force_complex=True)),
}
INVARIANCE_CASES = ("crosstalk", "leaky-2")


@functools.lru_cache(maxsize=None)
def scenario(name):
    make, args, kw = CASES[name]
    return make(*args), kw


def _take(c, idx):
    """Members idx of a scenario."""
    q = dict(c)
    q["z0"], q["op0"] = c["z0"][idx], c["op0"][idx]
    if np.ndim(c["model"]) == 3:
        q["model"] = c["model"][idx]
    return q


def open_observed(c, kw):
    clock = m4q.StepClock(c["dt"], c["T"], c["ns"])
    return open_session(c["z0"], c["model"], c["m"], 1, c["X_bm"], c["U_bm"], clock, c["op0"], c["ops"], c["Q"], c["R"], c["Q"],
                        c["sat"], c["du"], observe=c["kind"], **kw)


def collect(sess):
    res = sess.results()
    res["zs"] = sess.plant_states()
    res["path_detail"] = sess.path_detail()
    return res


def run_observed(c, kw, pieces=None):
    """Layout of the session's own arrays: xs [B, ns + 1, n], zs [B, ns + 1, n_p], us [B, ns, m]."""
    sess = open_observed(c, kw)
    try:
        for b, e in pieces or [(0, c["ns"])]:
            sess.run_observed(b, e)
        sess.sync()
        return collect(sess)
    finally:
        sess.close()


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One device-resident run per case, shared by the tests below (and left unchanged by them)."""
    c, kw = scenario(name)
    return run_observed(c, kw)


def host_loop(c, kw, z0):
    """Today's per-step host work around a PLANT_NONE session: launch, download the control, plant_step_batch, NumPy lift,
    put_state, sync.  The X0 field is the device's observation of z0, as the device-resident session's is: what is compared is
    the per-step work of the loop, not the lift of the first state."""
    B, n, m, ns = z0.shape[0], c["n"], c["m"], c["ns"]
    sess = EnsembleSession(B, n, m, 1, c["T"], ns, c["dt"], c["sat"], c["du"], plant_kind=_lib.PLANT_NONE,
                           target_cols=ns + c["T"] + 1, **kw)
    # (n_p = 9 has plant kernels for two controls only: H_X alone is stepped with a zero second operator, which adds exact zeros)
    ops, pad = c["ops"], 0
    if c["kind"] == QB and m == 1:
        ops, pad = np.concatenate([c["ops"], np.zeros_like(c["ops"])]), 1
    try:
        sess.load_problem(c["model"][None] if np.ndim(c["model"]) == 2 else c["model"], ob.observe_batch(c["kind"], z0), c["X_bm"],
                          c["U_bm"], c["Q"], c["R"], c["Q"])
        zs = np.zeros((B, ns + 1, z0.shape[1]), dtype=complex)
        zs[:, 0] = z0
        alive = np.ones(B, dtype=bool)
        for k in range(ns):
            sess.run(k, k + 1)
            sess.sync()
            alive &= sess.download(_lib.F_CODES, (B,)) == 0
            u = sess.download(_lib.F_US, (B, ns, m))[:, k]
            zn = m4q.plant_step_batch(zs[:, k], np.hstack([u, np.zeros((B, pad))]), c["op0"], ops, c["dt"])
            zs[alive, k + 1] = zn[alive]
            x_next = sess.get_state(k + 1)
            x_next[alive] = ob.observe_reference(c["kind"], zs[alive, k + 1])
            sess.put_state(k + 1, x_next)
        res = sess.results()
        res["zs"] = zs
        res["path_detail"] = sess.path_detail()
        return res
    finally:
        sess.close()


# ---------------------------------------------------------------- residuals of a run
@pytest.mark.parametrize("name", sorted(CASES))
def test_residuals_of_a_run(name):
    """In the run's own zs, us, xs - independent of the conditioning of the QPs: every completed step is one plant step and its
    observation."""
    c, _ = scenario(name)
    res = device_run(name)
    assert np.all(res["exit_codes"] == 0) and np.all(res["steps_done"] == c["ns"])
    assert np.array_equal(res["zs"][:, 0], c["z0"])
    worst_z = worst_x = 0.0
    for b in range(c["z0"].shape[0]):
        for k in range(c["ns"]):
            want = orc.plant_step(res["zs"][b, k], res["us"][b, k], c["op0"][b], list(c["ops"]), c["dt"])
            worst_z = max(worst_z, np.abs(res["zs"][b, k + 1] - want).max() / max(1.0, np.abs(want).max()))
    for k in range(c["ns"] + 1):
        worst_x = max(worst_x, lift_error(c["kind"], res["xs"][:, k], res["zs"][:, k]))
    print("%s: plant residual %.3e, lift residual %.3e" % (name, worst_z, worst_x))
    assert worst_z <= PLANT_TOL
    assert worst_x <= (0.0 if c["kind"] == PT else LIFT_TOL)
    assert np.abs(res["us"]).max() > 0.1 * c["sat"]               # the loop really drives


def test_crosstalk_member_against_the_oracle():
    """Member ct = 0.1 is the run of test_mpc_crosstalk_model_on_reduced_states: its bounds."""
    c, _ = scenario("crosstalk")
    res = device_run("crosstalk")
    b = 2
    exp = orc.OracleQCoupledExperiment(c["op0"][b], list(c["ops"]))
    (xo, uo), _, co = orc.mpc(c["z0"][b], 2, 1, c["X_bm"], c["U_bm"], orc.OracleClock(c["dt"], c["T"], c["ns"]), exp,
                              orc.OracleDMDc(8, 8, 16, c["model"]), c["Q"], c["R"], c["Q"], sat=c["sat"], du=c["du"])
    zs, us = res["zs"][b].T, res["us"][b].T
    assert co == 0 and zs.shape == xo.shape == (16, c["ns"] + 1) and us.shape == uo.shape
    print("crosstalk vs oracle: first steps us %.3e zs %.3e, whole run us %.3e zs %.3e"
          % (rel(us[:, :2], uo[:, :2]), rel(zs[:, :3], xo[:, :3]), rel(us, uo), rel(zs, xo)))
    assert rel(us[:, :2], uo[:, :2]) <= 1e-9 and rel(zs[:, :3], xo[:, :3]) <= 1e-9
    assert rel(us, uo) <= 1e-5 and rel(zs, xo) <= 1e-5


# ---------------------------------------------------------------- against the host path
def _movement(base, others):
    """Per step, how far the runs `others` are from `base`, never decreasing along the run: (controls [ns], states [ns + 1])."""
    eu = np.zeros(base["us"].shape[1])
    ex = np.zeros(base["xs"].shape[1])
    for o in others:
        eu = np.maximum(eu, np.maximum.accumulate(np.abs(o["us"] - base["us"]).max(axis=(0, 2))))
        ex = np.maximum(ex, np.maximum.accumulate(np.abs(o["xs"] - base["xs"]).max(axis=(0, 2))))
    return eu, ex


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_host_loop(name):
    c, kw = scenario(name)
    res = device_run(name)
    host = host_loop(c, kw, c["z0"])
    assert res["path_detail"] == host["path_detail"]
    assert np.array_equal(res["exit_codes"], host["exit_codes"]) and np.array_equal(res["steps_done"], host["steps_done"])
    assert np.array_equal(res["us"][:, 0], host["us"][:, 0])                      # step 0: the same launch on the same inputs
    eu, ex = _movement(host, [host_loop(c, kw, c["z0"] * s) for s in (1 + 1e-15, 1 - 1e-15)])
    du = np.abs(res["us"] - host["us"]).max(axis=(0, 2))
    dx = np.abs(res["xs"] - host["xs"]).max(axis=(0, 2))
    print("%s (%s): deviation from the host loop us %.3e xs %.3e zs %.3e; the host loop's own movement us %.3e xs %.3e"
          % (name, res["path_detail"], du.max(), dx.max(), np.abs(res["zs"] - host["zs"]).max(), eu.max(), ex.max()))
    assert np.all(du <= 100 * eu), (du, eu)
    assert np.all(dx <= 100 * ex), (dx, ex)


# ---------------------------------------------------------------- invariances (bit for bit)
def _same(a, b, keys=("xs", "zs", "us", "exit_codes", "steps_done", "qp_solves")):
    return [k for k in keys if not np.array_equal(a[k], b[k], equal_nan=True)]


@pytest.mark.parametrize("name", INVARIANCE_CASES)
def test_a_member_runs_the_same_alone(name):
    c, kw = scenario(name)
    res = device_run(name)
    for b in range(c["z0"].shape[0]):
        alone = run_observed(_take(c, [b]), kw)
        assert _same({k: v[b:b + 1] for k, v in res.items() if k != "path_detail"}, alone) == [], b


@pytest.mark.parametrize("name", INVARIANCE_CASES)
def test_split_runs_and_restore_continue_the_same_run(name):
    c, kw = scenario(name)
    res = device_run(name)
    assert _same(res, run_observed(c, kw, pieces=[(0, 3), (3, c["ns"])])) == []
    first = open_observed(c, kw)
    try:
        first.run_observed(0, 3)
        first.sync()
        state = first.state()
    finally:
        first.close()
    assert "zs" in state and np.all(state["zs"][:, 4:] == 0) and np.all(state["steps_done"] == 3)
    fresh = open_observed(c, kw)
    try:
        fresh.restore(state)
        fresh.run_observed(3, c["ns"])
        fresh.sync()
        got = collect(fresh)
        # (the solve counts of the steps before the checkpoint are a diagnostic of the session that ran them, not part of state())
        assert _same(res, got, keys=("xs", "zs", "us", "exit_codes", "steps_done")) == []
        assert np.array_equal(res["qp_solves"][:, 3:], got["qp_solves"][:, 3:])
    finally:
        fresh.close()


def test_state_carries_plant_states_only_with_an_observed_plant():
    c, kw = scenario("crosstalk")
    B, ns = c["z0"].shape[0], c["ns"]
    sess = EnsembleSession(B, 8, 2, 1, c["T"], ns, c["dt"], c["sat"], c["du"], plant_kind=_lib.PLANT_NONE, target_cols=ns + c["T"] + 1)
    try:
        assert "zs" not in sess.state()
        with pytest.raises(ValueError):
            sess.run_observed(0, 1)
    finally:
        sess.close()


# ---------------------------------------------------------------- a member that ends early
@pytest.mark.parametrize("name", INVARIANCE_CASES)
def test_a_member_that_ends_early_leaves_the_rest_alone(name):
    """(On the complex path: a NaN among the models disqualifies the whole upload from the real ones, so the run without it is
    taken on the same path.)"""
    c, kw = scenario(name)
    kw = dict(kw, force_complex=True)
    B = c["z0"].shape[0]
    q = dict(c)
    q["model"] = np.tile(c["model"][None], (B, 1, 1))
    rest = [0, 2, 3, 4]
    good = run_observed(_take(q, rest), kw)
    q["model"][1, 0, 0] = np.nan
    bad = run_observed(q, kw)
    assert bad["exit_codes"][1] == 3 and bad["steps_done"][1] == 0
    assert np.array_equal(bad["zs"][1, 0], c["z0"][1]) and np.all(bad["zs"][1, 1:] == 0)
    assert np.all(good["exit_codes"] == 0) and np.all(good["steps_done"] == c["ns"])
    assert _same(good, {k: v[rest] for k, v in bad.items() if k != "path_detail"}) == []


# ---------------------------------------------------------------- refusals on a live session
def test_capi_refusals_on_a_live_session():
    c, kw = scenario("crosstalk")
    B, ns = c["z0"].shape[0], c["ns"]
    L = _lib.lib()
    _, z0 = _lib.cbuf(c["z0"])
    _, op0 = _lib.cbuf(c["op0"])
    _, ops = _lib.cbuf(c["ops"])

    def session(n=8, m=2, **more):
        return EnsembleSession(B, n, m, 1, c["T"], ns, c["dt"], c["sat"], c["du"], target_cols=ns + c["T"] + 1, **more)
    for sess, kind in ((session(n=4, plant_kind=_lib.PLANT_HAMILTONIAN), QB), (session(plant_kind=_lib.PLANT_NONE, measure_freq=2), PT),
                       (session(plant_kind=_lib.PLANT_NONE), QB), (session(n=4, plant_kind=_lib.PLANT_NONE), PT),
                       (session(plant_kind=_lib.PLANT_NONE), 3)):
        try:
            assert L.m4q_session_set_observed_plant(sess._h, kind, op0, ops, 1, z0) == _lib.E_BADARG
            assert L.m4q_session_run_observed(sess._h, 0, 1) == _lib.E_BADARG          # nothing was set
        finally:
            sess.close()
    sess = open_observed(c, kw)
    try:
        for args in ((None, ops, z0), (op0, None, z0), (op0, ops, None)):
            assert L.m4q_session_set_observed_plant(sess._h, PT, args[0], args[1], 1, args[2]) == _lib.E_BADARG
        for b, e in ((-1, 1), (0, ns + 1), (2, 2), (3, 1)):
            assert L.m4q_session_run_observed(sess._h, b, e) == _lib.E_BADARG
        buf = np.zeros((B, ns + 1, 16), dtype=complex)
        assert L.m4q_session_plant_states(sess._h, buf.ctypes.data, buf.nbytes - 16) == _lib.E_BADARG
        assert L.m4q_session_put_plant_states(sess._h, buf.ctypes.data, buf.nbytes + 16) == _lib.E_BADARG
        # noise and exit conditions stay refused, as on every PLANT_NONE session
        _, sigma = _lib.rbuf(np.array([1e-3]))
        assert L.m4q_session_set_noise(sess._h, _lib.NOISE_IID, sigma, 0, 1, 0) == _lib.E_BADARG
        _, W = _lib.cbuf(np.eye(8))
        _, thr = _lib.rbuf(np.array([0.1]))
        assert L.m4q_session_set_exit(sess._h, _lib.EXIT_NEXT | _lib.EXIT_BELOW, W, W, 0, thr, 0) == _lib.E_UNSUPPORTED
        sess.run_observed(0, 1)
        sess.sync()
        assert L.m4q_session_set_observed_plant(sess._h, PT, op0, ops, 1, z0) == _lib.E_BADARG       # after the first run
    finally:
        sess.close()
    # the plant kinds stay what they were: no kind above 3 anywhere else
    with pytest.raises(_lib.M4qError):
        m4q.plant_step_batch(c["z0"], np.zeros((B, 2)), c["op0"], c["ops"], c["dt"], kind=4)


# ---------------------------------------------------------------- mpc() as a drop-in
class _HostCoupled(m4q.QCoupledExperiment):
    """The same lift, overridden: mpc() takes the host path for it."""

    @staticmethod
    def lift(v):
        return m4q.QCoupledExperiment.lift(v)


class _HostLeaky(m4q.QExperiment32):
    @staticmethod
    def lift(v):
        return m4q.QExperiment32.lift(v)


@pytest.fixture
def launches(monkeypatch):
    """Which of the two session entry points mpc() used."""
    seen = []
    for name in ("run", "run_observed"):
        orig = getattr(EnsembleSession, name)

        def spy(self, b=0, e=None, _orig=orig, _name=name):
            seen.append((_name, b, e))
            return _orig(self, b, e)
        monkeypatch.setattr(EnsembleSession, name, spy)
    return seen


@pytest.mark.parametrize("name, cls, host_cls, n_p", [("crosstalk", m4q.QCoupledExperiment, _HostCoupled, 16),
                                                      ("leaky-2", m4q.QExperiment32, _HostLeaky, 9)])
def test_mpc_dropin(name, cls, host_cls, n_p, launches):
    c, _ = scenario(name)
    b = 2
    n, m, ns = c["n"], c["m"], c["ns"]

    def run(exp_cls, scale=1.0):
        clock = m4q.StepClock(c["dt"], c["T"], ns)
        exp = exp_cls(c["op0"][b], list(c["ops"]))
        (xs, us), _, code = m4q.mpc(c["z0"][b] * scale, m, 1, c["X_bm"], c["U_bm"], clock, exp, m4q.DMDc(n, n, n * m, c["model"]),
                                    c["Q"], c["R"], c["Q"], sat=c["sat"], du=c["du"], progress_bar=False)
        assert code == 0 and len(clock.ts_sim) == ns
        return dict(xs=xs.T[None], us=us.T[None])
    dev = run(cls)
    assert launches == [("run_observed", 0, ns)]
    del launches[:]
    host = run(host_cls)
    assert [l[0] for l in launches] == ["run"] * ns
    assert dev["xs"].shape == (1, ns + 1, n_p) and dev["us"].shape == (1, ns, m)
    assert np.array_equal(dev["xs"][0, 0], c["z0"][b])
    eu, ex = _movement(host, [run(host_cls, s) for s in (1 + 1e-15, 1 - 1e-15)])
    du = np.abs(dev["us"] - host["us"]).max(axis=(0, 2))
    dx = np.abs(dev["xs"] - host["xs"]).max(axis=(0, 2))
    print("mpc() %s: deviation from the host path us %.3e xs %.3e; the host path's own movement us %.3e xs %.3e"
          % (name, du.max(), dx.max(), eu.max(), ex.max()))
    assert np.all(du <= 100 * eu), (du, eu)
    assert np.all(dx <= 100 * ex), (dx, ex)
    # the same member of the ensemble run, bit for bit in the controls the QPs chose
    assert np.array_equal(dev["us"][0], device_run(name)["us"][b])

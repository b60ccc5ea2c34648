"""Measurement noise drawn on the device inside the fused loop (-m gpu): m4q_noise_sample_batch against the NumPy replica
(mpc4quantum_amd/noise.py), the noise found in a closed loop's own stored states, teacher-forced steps against the oracle with a
noisy plant, independence from the launch schedule, the placement in a batch and the sharding, off means off, exit conditions
that read the noisy state, the drop-in mpc() and the refusals of the C ABI.

The oracle takes an experiment object: the noisy oracle plants below are subclasses of the oracle's plants whose simulate() adds
MeasurementNoise.sample for the column of xs the step writes (ts[-1] / dt = step + 1)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from mpc4quantum_amd.mpc import open_session
from oracle import m4q_oracle as orc
from tests import kernel_variants as kv
from tests.test_gpu_launch_schedule import _agree, _same, _snapshot, _take
from tests.test_gpu_variant_matrix import _open

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("iid", "hermitian")
PATH_KW = {kv.COMPLEX: dict(force_complex=True), kv.REAL: dict(traceless=False), kv.TRACELESS: dict(tile=False, shared_generators=False),
           kv.TILE: dict(tile=True), kv.SG: dict()}


def plant_tol(x):
    """The project's plant tolerance: 1e-10 max(1, |x|_inf)."""
    return 1e-10 * max(1.0, float(np.abs(x).max()))


# ---------------------------------------------------------------- noisy oracle plants
class _Noisy:
    """simulate() of the oracle's plant plus the draws of (member, column of xs = ts[-1] / dt): only the last column - the
    measured state - is used by the loop (mpc.py:259-260), and only it gets noise."""

    def with_noise(self, noise, member, dt):
        self.noise, self.member, self.dt = noise, int(member), float(dt)
        return self

    def simulate(self, x0, ts, u_fn):
        res = np.array(super().simulate(x0, ts, u_fn))
        res[:, -1] += self.noise.sample([self.member], int(round(ts[-1] / self.dt)), res.shape[0])[0]
        return res


class NoisyOracleQExperiment(_Noisy, orc.OracleQExperiment):
    pass


class NoisyOracleLExperiment(_Noisy, orc.OracleLExperiment):
    pass


def noisy_oracle_run(p, b, noise, stop=None, start=None, trace=None, count=None, exit_condition=None, measure_freq=1):
    """oracle.mpc of member b of scenario p (Hamiltonian plant) under `noise`."""
    n = p["dim_x"]
    Am = p["models"][b if p["models"].shape[0] > 1 else 0]
    model = orc.OracleDMDc(n, n, Am.shape[1] - n, Am)
    exp = NoisyOracleQExperiment(p["plant_op0"][b if p["plant_op0"].shape[0] > 1 else 0], list(p["plant_ops"][0]))
    exp.with_noise(noise, b, p["dt"])
    clock = orc.OracleClock(p["dt"], p["horizon"], p["n_steps"])
    clock.measure_freq = measure_freq
    return orc.mpc(p["x0"][b], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, exp, model, p["Q"], p["R"], p["Qf"],
                   sat=p["sat"], du=p["du"], start=start, stop=stop, trace=trace, count=count, exit_condition=exit_condition)


def noisy_step_sensitivity(p, b, k, xs, us, guess, noise):
    """tests/test_gpu_parity.py::_oracle_step_sensitivity with the noisy plant: how far the ORACLE's us[k], xs[k + 1] and the
    guesses it leaves behind move when the SQP guess step k starts from is perturbed by a few 1e-15 (xs (n, ns + 1), us (m, ns))."""
    outs = []
    for eps in (0.0, 1e-15, -1e-15, 3e-15):
        tr = []
        st = dict(step=k, xs=xs, us=us, X_guess=guess[0] * (1 + eps), U_guess=guess[1])
        (x2, u2), _, _ = noisy_oracle_run(p, b, noise, stop=k + 1, start=st, trace=tr)
        outs.append((u2[:, k], x2[:, k + 1], tr[-1][0], tr[-1][1]))
    return [max(np.abs(o[i] - outs[0][i]).max() for o in outs[1:]) for i in range(4)]


# ---------------------------------------------------------------- 1. generator parity
def device_sample(B, n, noise, state_index):
    out = np.empty((B, n), dtype=np.complex128)
    sg = np.ascontiguousarray(noise.sigma, dtype=np.float64).reshape(-1)
    _lib.check(_lib.lib().m4q_noise_sample_batch(B, n, noise.mode, sg.ctypes.data_as(_lib._dp), int(noise.sigma.ndim == 1), noise.seed,
                                                 noise.member_base, int(state_index), out.ctypes.data_as(_lib._dp)))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [4, 9, 16])
def test_generator_parity_with_the_replica(n, kind, record_property):
    """m4q_noise_sample_batch against noise.py.  The integer stage is identical by construction, so any difference comes from
    log / sqrt / sincos: 1e-13 absolute on unit z (|z| <= 8.57 and a few ulps of the device library give about 1e-14; a factor of
    ten is left).  The Hermitian kind is a combination of the z with absolute row sum 2 (1 - 1/d) < 2 on the diagonal and 1 off it:
    twice the bound.  Members straddle 2^32 (the second counter word), seeds use both key words."""
    B, base, seed = 131, (1 << 32) - 67, 0xA4093822299F31D0
    lin = 2.0 if kind == "hermitian" else 1.0
    worst = 0.0
    for sidx in (1, 2, 20, 65537):
        unit = m4q.MeasurementNoise(1.0, seed, kind, member_base=base)
        got = device_sample(B, n, unit, sidx)
        err = np.abs(got - unit.sample(np.arange(B), sidx, n)).max()
        worst = max(worst, err / lin)
        print("n=%d %s state_index=%d max|device - replica| = %.3e" % (n, kind, sidx, err))
        assert err <= lin * 1e-13, (sidx, err)
        if kind == "iid":
            assert np.abs(got - unit.unit(np.arange(B), sidx, n)).max() <= 1e-13
        else:
            G = got.reshape(B, int(np.sqrt(n)), -1)
            assert np.array_equal(G, np.conj(np.swapaxes(G, 1, 2)))                    # Hermitian exactly, on the device too
        sigma = np.linspace(0.0, 3.0, B)
        per = m4q.MeasurementNoise(sigma, seed, kind, member_base=base)
        got = device_sample(B, n, per, sidx)
        want = per.sample(np.arange(B), sidx, n)
        assert np.all(np.abs(got - want) <= lin * 1e-13 * sigma[:, None]), sidx
        assert np.all(got[0] == 0)
    record_property("max_unit_error", worst)
    # a block of the members equals the rows of the whole (member_base)
    whole = device_sample(B, n, m4q.MeasurementNoise(0.5, seed, kind, member_base=base), 3)
    part = device_sample(9, n, m4q.MeasurementNoise(0.5, seed, kind, member_base=base + 60), 3)
    assert _same(part, whole[60:69])


# ---------------------------------------------------------------- 2. the noise residual of a closed loop
def _residual_case(cfg, order=1):
    if cfg == "gen":
        p = kv.scenario(9, 2, 1, batch=3, horizon=8, n_steps=6)
        return p, _lib.PLANT_GENERATOR, p["gen_op0"], p["gen_ops"]
    if cfg == "synthesis":
        p = kv.process_scenario(1, 1, batch=3, horizon=8, n_steps=6)
        return p, _lib.PLANT_PROCESS, p["plant_op0"], np.broadcast_to(p["plant_ops"], (3,) + p["plant_ops"].shape[1:])
    p = configs.build(cfg, batch=3, order=order, horizon=8, n_steps=6)
    return p, _lib.PLANT_HAMILTONIAN, p["plant_op0"], p["plant_ops"]


def _clean_plant(p, kind_code, b):
    """The oracle's noise-free plant of member b."""
    if kind_code == _lib.PLANT_HAMILTONIAN:
        return orc.OracleQExperiment(p["plant_op0"][b if p["plant_op0"].shape[0] > 1 else 0], list(p["plant_ops"][0]))
    g0 = p["gen_op0"]
    return orc.OracleLExperiment(g0[b if g0.shape[0] > 1 else 0], list(p["gen_ops"][0]))


def _check_residuals(p, kind_code, res, noise, mf):
    """Every measured step: xs[k + 1] - plant(xs[k + 1 - mf]; the replayed controls) = noise.sample(member, k + 1); every other
    step: xs[k + 1] = the model's prediction from xs[k].  Both to the plant tolerance, on the device's own xs and us."""
    B, n, m, ns = p["batch"], p["dim_x"], p["dim_u"], p["n_steps"]
    xs, us = res["xs"], res["us"]                                      # time-major [B, ns + 1, n], [B, ns, m]
    clock = orc.OracleClock(p["dt"], p["horizon"], ns)
    clock.measure_freq = mf
    worst = 0.0
    for b in range(B):
        plant = _clean_plant(p, kind_code, b)
        Am = p["models"][b if p["models"].shape[0] > 1 else 0]
        model = orc.OracleDMDc(n, n, Am.shape[1] - n, Am)
        wm = orc.OracleWrapModel(*model.get_discrete(), m, p["order"])
        for k in range(ns):
            if (k + 1) % mf == 0:
                us_step = np.vstack([us[b, k - jq] for jq in range(mf)] + [us[b, k]]).T      # newest first (mpc.py:257)
                clean = plant.simulate(xs[b, k + 1 - mf], clock.ts_step(k), us_step)[:, -1]
                want = noise.sample([b], k + 1, n)[0]
            else:
                lx = xs[b, k].reshape(-1, 1)
                clean = np.reshape(model.predict(lx, orc.krtimes(wm.lift_u(us[b, k].reshape(-1, 1)), lx)), -1)
                want = np.zeros(n)
            err = np.abs(xs[b, k + 1] - clean - want).max()
            worst = max(worst, err / plant_tol(xs[b, k + 1]))
            assert err <= plant_tol(xs[b, k + 1]), (b, k, err)
    return worst


RESIDUAL_CASES = (
    [(cfg, "iid", kv.COMPLEX) for cfg in (1, 2, 3, 4, "gen", "synthesis")] +
    [(cfg, "hermitian", path) for cfg in (1, 2, 3) for path in (kv.COMPLEX, kv.REAL, kv.TRACELESS, kv.TILE)] +
    [(4, "hermitian", path) for path in (kv.COMPLEX, kv.REAL, kv.TRACELESS, kv.SG)] +
    [("gen", "hermitian", kv.TILE)])


@pytest.mark.parametrize("mf", [1, 2])
@pytest.mark.parametrize("cfg,kind,path", RESIDUAL_CASES, ids=lambda v: str(v))
def test_noise_residual_in_the_closed_loop(cfg, kind, path, mf, record_property):
    """The primary parity check; it does not depend on how well conditioned the QP is.  One fused launch with noise on; the
    residual of the device's own stored xs against the oracle's plant from the device's own stored states and controls is the
    replica's noise, per member and step, on every arithmetic path the case supports (path_detail() asserted; "iid" runs the
    complex path without being forced to).  Per-member sigma."""
    p, kind_code, op0, ops = _residual_case(cfg)
    B = p["batch"]
    noise = m4q.MeasurementNoise(np.array([1e-2, 3e-3, 2e-2]), seed=0x1234567887654321 + mf, kind=kind, member_base=(1 << 32) - 1)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    clock.measure_freq = mf
    kw = dict(PATH_KW[path]) if kind == "hermitian" else {}
    sg = path == kv.SG
    if sg:
        kw.update(generators=p["generators"], scales=p["scales"])
    sess = open_session(p["x0"], None if sg else p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, op0, ops, p["Q"],
                        p["R"], p["Qf"], p["sat"], p["du"], plant_kind=kind_code, noise=noise, **kw)
    try:
        assert sess.path_detail() == path
        sess.run(0, p["n_steps"])
        res = sess.results()
        assert sess.path_detail() == path
    finally:
        sess.close()
    assert np.all(res["exit_codes"] == 0) and np.all(res["steps_done"] == p["n_steps"]), (res["exit_codes"], res["steps_done"])
    local = m4q.MeasurementNoise(noise.sigma, noise.seed, kind, member_base=noise.member_base)
    worst = _check_residuals(p, kind_code, res, local, mf)
    record_property("worst_residual_over_tolerance", worst)
    # the noise is there: a measured state differs from the clean plant by about sigma
    assert np.abs(res["xs"][:, mf] - _clean_first(p, kind_code, res, mf)).max() > 1e-4


def _clean_first(p, kind_code, res, mf):
    clock = orc.OracleClock(p["dt"], p["horizon"], p["n_steps"])
    clock.measure_freq = mf
    k = mf - 1
    out = []
    for b in range(p["batch"]):
        us_step = np.vstack([res["us"][b, k - jq] for jq in range(mf)] + [res["us"][b, k]]).T
        out.append(_clean_plant(p, kind_code, b).simulate(res["xs"][b, 0], clock.ts_step(k), us_step)[:, -1])
    return np.stack(out)


# ---------------------------------------------------------------- 3. controls: teacher-forced steps against the noisy oracle
# (config, order, batch, horizon; None = the configuration's own T).  Config 3 at its own T = 40 is not among them: its oracle moves
# by 4.7e-11 on us[k] under a 1e-15 perturbation of the guess with NO noise at all (3.4e-11 with it) - over the 1e-12 the cases must
# meet.  At T = 16 (the horizon test_closed_loop_vs_oracle runs it at) it moves by 3e-14.
CONTROL_CASES = [(1, 1, 1, None), (1, 2, 1, None), (2, 1, 3, None), (3, 1, 4, 16)]
SIGMA_CONTROLS = 1e-3


def control_case(cfg, order, batch, horizon, kind):
    p = configs.build(cfg, batch=max(batch, 4) if cfg == 3 else batch, order=order, horizon=horizon)
    q = dict(p, batch=batch, x0=p["x0"][:batch], models=p["models"] if p["models"].shape[0] == 1 else p["models"][:batch])
    noise = m4q.MeasurementNoise(SIGMA_CONTROLS, seed=20240917 + 10 * cfg + order, kind=kind)
    return q, noise


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg,order,batch,horizon", CONTROL_CASES)
def test_controls_teacher_forced_against_the_noisy_oracle(cfg, order, batch, horizon, kind, record_property):
    """Every MPC step started from the noisy ORACLE's state (states, controls, SQP guesses) through the checkpoint fields, as
    tests/test_gpu_parity.py::test_closed_loop_stepwise_teacher_forced does: us[k] and xs[k + 1] to the fixed 1e-10, identical
    QP-solve counts, NO sensitivity clause.  The cases are the ones whose oracle moves by at most 1e-12 on us[k] and xs[k + 1] when
    the guess a step starts from is perturbed by 1e-15 (noisy_step_sensitivity, asserted here on every step): configs 1 (orders 1,
    2) and 2 at their own horizons and config 3 at T = 16, sigma = 1e-3, both kinds ("hermitian" on the path the configuration
    gets by default, "iid" on the complex path)."""
    p, noise = control_case(cfg, order, batch, horizon, kind)
    ns = p["n_steps"]
    runs = []
    for b in range(batch):
        tr, cnt = [], []
        (xs, us), _, code = noisy_oracle_run(p, b, noise, trace=tr, count=cnt)
        assert code == 0
        runs.append((xs, us, tr, cnt))
    xs_t = np.stack([r[0].T for r in runs])
    us_t = np.stack([r[1].T for r in runs])
    solves = np.array([r[3] for r in runs])
    sens = np.max([[noisy_step_sensitivity(p, b, k, runs[b][0], runs[b][1], runs[b][2][k], noise)[:2] for k in range(ns)]
                   for b in range(batch)], axis=(0, 1))
    print("oracle step sensitivity (us[k], xs[k+1]) max over steps and members: %s" % sens)
    assert np.all(sens <= 1e-12), sens
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    sess = open_session(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"],
                        p["Q"], p["R"], p["Qf"], p["sat"], p["du"], noise=noise)
    worst = [0.0, 0.0]
    try:
        want = kv.COMPLEX if kind == "iid" else (kv.TILE if order == 1 else kv.TRACELESS)
        assert sess.path_detail() == want
        for k in range(ns):
            if k > 0:
                st = {"xs": np.zeros_like(xs_t), "us": np.zeros_like(us_t),
                      "x_guess": np.stack([runs[b][2][k][0].T for b in range(batch)]),
                      "u_guess": np.stack([runs[b][2][k][1].T for b in range(batch)]),
                      "exit_codes": np.zeros(batch, dtype=np.int32), "steps_done": np.full(batch, k, dtype=np.int32)}
                st["xs"][:, :k + 1] = xs_t[:, :k + 1]
                st["us"][:, :k] = us_t[:, :k]
                sess.restore(st)
            sess.run(k, k + 1)
            got = sess.state()
            assert np.array_equal(sess.download(_lib.F_QP_SOLVES, (batch, ns))[:, k], solves[:, k]), k
            eu = np.abs(got["us"][:, k] - us_t[:, k]).max() / max(1.0, np.abs(us_t[:, k]).max())
            ex = np.abs(got["xs"][:, k + 1] - xs_t[:, k + 1]).max() / max(1.0, np.abs(xs_t[:, k + 1]).max())
            worst = [max(worst[0], eu), max(worst[1], ex)]
            print("step %2d: us %.3e xs %.3e" % (k, eu, ex))
            assert eu <= 1e-10 and ex <= 1e-10, (k, eu, ex)
            assert np.all(got["steps_done"] == k + 1) and np.all(got["exit_codes"] == 0)
    finally:
        sess.close()
    record_property("worst_us_xs", worst)


# ---------------------------------------------------------------- 4. schedule independence
NS = kv.LONG_STEPS
SCHEDULE_CELLS = [(kv.LoopCell(9, 2, 1, kv.COMPLEX, False, kv.HAMILTONIAN), "iid"),
                  (kv.LoopCell(9, 2, 1, kv.COMPLEX, False, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(9, 2, 1, kv.REAL, False, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(9, 2, 1, kv.TRACELESS, False, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(9, 2, 1, kv.TILE, False, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(9, 2, 1, kv.TRACELESS, True, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(9, 2, 1, kv.COMPLEX, True, kv.HAMILTONIAN), "iid"),
                  (kv.LoopCell(16, 3, 1, kv.SG, False, kv.HAMILTONIAN), "hermitian"),
                  (kv.LoopCell(16, 1, 1, kv.COMPLEX, False, kv.PROCESS), "iid")]


def _sched_id(v):
    return kv.cell_id(v) if isinstance(v, kv.LoopCell) else str(v)


def _schedule_scenario(cell, batch=kv.BATCH):
    if cell.plant == kv.PROCESS:
        return kv.process_scenario(cell.nu, cell.order, batch=batch, n_steps=NS)
    return kv.scenario(cell.nx, cell.nu, cell.order, batch=batch, n_steps=NS)


@pytest.mark.parametrize("cell,kind", SCHEDULE_CELLS, ids=_sched_id)
def test_noise_is_independent_of_the_launch_schedule(cell, kind):
    """One launch of all 14 steps against a chain of single-step launches, a two-launch resume at every cut of
    kernel_variants.pieces (and one step either side), and a checkpoint restored into a fresh session that is given the same
    noise: identical bits on the complex path, the real-path bounds of tests/test_gpu_launch_schedule.py otherwise (_agree); the
    restored session equals the same-session resume bit for bit on every path."""
    p = _schedule_scenario(cell)
    B = p["batch"]
    noise = m4q.MeasurementNoise(np.linspace(1e-3, 5e-3, B), seed=77, kind=kind, member_base=123456789012)
    cuts = sorted({c + o for (lo, hi) in kv.pieces(0, NS, cell.exact)[1:] for c in (lo,) for o in (-1, 0, 1)})
    worst = [0.0, 0.0]
    resumed, checkpoints = {}, {}
    sess = _open(cell, p)
    try:
        sess.set_noise(noise)
        assert sess.path_detail() == cell.path
        sess.run(0, NS)
        ref = _snapshot(sess)
        assert np.all(ref["exit_codes"] == 0) and np.all(ref["steps_done"] == NS), (ref["exit_codes"], ref["steps_done"])
        for k in range(NS):
            sess.run(k, k + 1)
        _agree(cell, ref, _snapshot(sess), "single steps", worst)
        for k in cuts:
            sess.run(0, k)
            if k in (2, 7):
                checkpoints[k] = (sess.state(), sess.download(_lib.F_QP_SOLVES, (B, NS)))
            sess.run(k, NS)
            resumed[k] = _snapshot(sess)
            _agree(cell, ref, resumed[k], "resumed at %d" % k, worst)
    finally:
        sess.close()
    # the noise is in the run: the same session without it lands elsewhere
    for k, (st, solves) in checkpoints.items():
        fresh = _open(cell, p)
        try:
            fresh.set_noise(noise)
            fresh.restore(st)
            fresh.upload(_lib.F_QP_SOLVES, solves)
            fresh.run(k, NS)
            got = _snapshot(fresh)
            assert fresh.path_detail() == cell.path
        finally:
            fresh.close()
        for f in got:
            assert _same(got[f], resumed[k][f]), (k, f)
    quiet = _open(cell, p)
    try:
        quiet.run(0, NS)
        off = _snapshot(quiet)
    finally:
        quiet.close()
    assert np.abs(off["xs"][:, 1] - ref["xs"][:, 1]).max() > 1e-5


BIG = 16 * 256 + 3
PLACES = (0, 1234, BIG - 5, BIG - 2, BIG - 1)


@pytest.mark.parametrize("cell,kind", [SCHEDULE_CELLS[0], SCHEDULE_CELLS[4], SCHEDULE_CELLS[5]], ids=_sched_id)
def test_noise_follows_the_member_not_its_place(cell, kind, monkeypatch):
    """Five members among 4,099 on a grid of one workgroup per CU (M4Q_WGS_PER_CU=1: every resident row runs member after member,
    the pieces of one member on different rows) against each of them alone (B = 1, member_base = its index): bit for bit."""
    monkeypatch.setenv("M4Q_WGS_PER_CU", "1")
    steps = 8
    p = kv.scenario(cell.nx, cell.nu, cell.order, batch=BIG, n_steps=steps)
    sigma = np.linspace(1e-3, 1e-2, BIG)
    sess = _open(cell, p)
    try:
        sess.set_noise(m4q.MeasurementNoise(sigma, seed=5, kind=kind, member_base=1 << 40))
        assert sess.path_detail() == cell.path and BIG >= 16 * sess.info()["grid"]
        sess.run(0, steps)
        big = _snapshot(sess)
    finally:
        sess.close()
    assert np.all(big["exit_codes"] == 0)
    for i in PLACES:
        one = _open(cell, _take(p, [i]), model_per_instance=True)
        try:
            one.set_noise(m4q.MeasurementNoise(sigma[i], seed=5, kind=kind, member_base=(1 << 40) + i))
            assert one.path_detail() == cell.path
            one.run(0, steps)
            alone = _snapshot(one)
        finally:
            one.close()
        for f in big:
            assert _same(alone[f][0], big[f][i]), (i, f)


# ---------------------------------------------------------------- 5. sharding
@pytest.mark.parametrize("kind", KINDS)
def test_sharded_two_ranks_draw_the_unsharded_noise(kind, tmp_path):
    """The two-ranks-on-one-GPU pattern of test_mpc_batch_sharded_two_ranks_on_one_gpu: 11 members as 6 + 5 with a per-member
    sigma; bit for bit the unsharded mpc_batch with the same noise."""
    script = tmp_path / "sharded_noise.py"
    script.write_text('''
import os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import torch.distributed as dist
import mpc4quantum_amd as m4q
from mpc4quantum_amd import configs
from mpc4quantum_amd.distributed import mpc_batch_sharded, shard_bounds
from gloo_transport import GlooTransport
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", rank=rank, world_size=2)
p = configs.build(3, batch=11, horizon=12, n_steps=6)
noise = m4q.MeasurementNoise(np.linspace(1e-3, 1e-2, 11), seed=424242, kind=%r, member_base=(1 << 32) - 8)
def clock(): return m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
args = lambda: (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock(), p["plant_op0"], p["plant_ops"],
                p["Q"], p["R"], p["Qf"], p["sat"], p["du"])
assert [shard_bounds(11, r, 2) for r in range(2)] == [(0, 6), (6, 11)]
got = mpc_batch_sharded(*args(), transport=GlooTransport(), noise=noise)
if rank == 0:
    ref = m4q.mpc_batch(*args(), noise=noise)
    quiet = m4q.mpc_batch(*args())
    for k in ("xs", "us", "exit_codes", "steps_done", "qp_solves"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert np.abs(ref["xs"] - quiet["xs"]).max() > 1e-4
else:
    assert got is None
dist.barrier()
dist.destroy_process_group()
print("rank %%d ok" %% rank)
''' % (ROOT, ROOT, kind))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547" if kind == "iid" else "29549", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(2)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=600))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, (pr, (so, se)) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0 and ("rank %d ok" % r) in so, so[-2000:] + se[-4000:]


# ---------------------------------------------------------------- 6. off means off
@pytest.mark.parametrize("cell", [kv.LoopCell(9, 2, 1, kv.TILE, False, kv.HAMILTONIAN), kv.LoopCell(9, 2, 1, kv.COMPLEX, False, kv.HAMILTONIAN),
                                  kv.LoopCell(16, 3, 1, kv.SG, False, kv.HAMILTONIAN), kv.LoopCell(4, 1, 1, kv.TRACELESS, True, kv.HAMILTONIAN)],
                         ids=kv.cell_id)
def test_off_means_off(cell):
    """A session that never calls set_noise, one that sets mode 0 and one that sets and then clears a noise: identical bits.
    "hermitian" with sigma = 0 equals noise off as numbers on the same path (-0.0 + 0.0 may flip a sign bit), "iid" with sigma = 0
    equals a forced-complex run."""
    p = kv.scenario(cell.nx, cell.nu, cell.order, n_steps=6)

    def run(prepare, c=cell):
        sess = _open(c, p)
        try:
            prepare(sess)
            path = sess.path_detail()
            sess.run(0, 6)
            return _snapshot(sess), path
        finally:
            sess.close()

    def set_and_clear(s):
        s.set_noise(m4q.MeasurementNoise(0.1, 3, "hermitian"))
        s.set_noise(None)

    never, path0 = run(lambda s: None)
    assert path0 == cell.path
    for prepare in (lambda s: s.set_noise(None), set_and_clear):
        got, path = run(prepare)
        assert path == cell.path
        for f in never:
            assert _same(got[f], never[f]), f
    zero, path = run(lambda s: s.set_noise(m4q.MeasurementNoise(0.0, 3, "hermitian")))
    assert path == cell.path
    for f in never:
        assert np.array_equal(zero[f], never[f]), f
    forced, pathc = run(lambda s: None, cell._replace(path=kv.COMPLEX))
    iid0, path = run(lambda s: s.set_noise(m4q.MeasurementNoise(np.zeros(p["batch"]), 3, "iid")))
    assert path == pathc == kv.COMPLEX
    for f in forced:
        assert np.array_equal(iid0[f], forced[f]), f


# ---------------------------------------------------------------- 7. exit conditions see the noisy state
@pytest.mark.parametrize("kind", KINDS)
def test_exit_condition_reads_the_noisy_state(kind):
    """A QuadraticExit on "next" on one coherence of config 3 (rho_02), which the noise (sigma = 2e-2) moves by as much as the
    steps do.  Per member the threshold sits midway between the largest value and the runner-up of the noisy ORACLE's run, so the
    condition fires at the step of the largest - in the oracle's run with the condition, and on the device.  The same condition
    without the noise decides otherwise for some member: the kernel read the noisy state."""
    p = configs.build(3, batch=4, horizon=12, n_steps=8)
    B, n, ns = 4, p["dim_x"], p["n_steps"]
    noise = m4q.MeasurementNoise(2e-2, seed=31337, kind=kind)
    W = np.zeros((n, n))
    W[2, 2] = 1.0
    thr, want = np.zeros(B), np.zeros(B, dtype=int)
    for b in range(B):
        (xs, _), _, code = noisy_oracle_run(p, b, noise)
        assert code == 0
        q = np.sort(np.abs(xs[2, 1:]) ** 2)                        # q of xs[k + 1], k = 0..ns-1
        thr[b] = 0.5 * (q[-1] + q[-2])
        want[b] = int(np.argmax(np.abs(xs[2, 1:]) ** 2 > thr[b]))
        assert q[-1] - q[-2] > 1e-6                                # far above what a free run of 8 steps differs by (1e-8)
    cond = m4q.QuadraticExit(W, np.zeros(n), thr, state="next", fires="above")
    for b in range(B):
        (xo, _), _, code = noisy_oracle_run(p, b, noise, exit_condition=lambda xn, x, u, b=b: cond(xn, x, u, member=b))
        assert code == 1 and xo.shape[1] == want[b] + 1, (b, code, xo.shape, want[b])
    clock = m4q.StepClock(p["dt"], p["horizon"], ns)
    args = (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"], p["R"],
            p["Qf"], p["sat"], p["du"])
    res = m4q.mpc_batch(*args, exit_condition=cond, noise=noise)
    assert np.all(res["exit_codes"] == 1) and np.array_equal(res["steps_done"], want), (res["exit_codes"], res["steps_done"], want)
    quiet = m4q.mpc_batch(*args, exit_condition=cond)
    assert not (np.array_equal(quiet["exit_codes"], res["exit_codes"]) and np.array_equal(quiet["steps_done"], res["steps_done"]))


# ---------------------------------------------------------------- 8. drop-in mpc()
@pytest.fixture
def launches(monkeypatch):
    seen = []
    orig = m4q.EnsembleSession.close

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            seen.append(self.kernel_ms()[1])
        return orig(self)
    monkeypatch.setattr(m4q.EnsembleSession, "close", close)
    return seen


@pytest.mark.parametrize("kind", KINDS)
def test_mpc_dropin_with_device_noise(kind, launches):
    """experiment.set_noise keeps mpc() fused - one launch - and agrees with the stepwise path (a plain-callable exit condition
    that never fires: one launch per step, the same draws added by mpc() itself) and with the noisy oracle, under the comparison
    of test_mpc_dropin_fused_equals_host_plant_and_oracle (1e-8 on an 8-step run); set_sigma alone still takes the host path."""
    p = configs.build(3, batch=1, horizon=12, n_steps=8)
    n, m = p["dim_x"], p["dim_u"]
    model = m4q.DMDc(n, n, p["models"].shape[2] - n, p["models"][0])
    noise = m4q.MeasurementNoise(5e-3, seed=99, kind=kind, member_base=7)

    def run(exp, **kw):
        clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
        return m4q.mpc(p["x0"][0], m, p["order"], p["X_targ"], p["U_targ"], clock, exp, model, p["Q"], p["R"], p["Qf"],
                       sat=p["sat"], du=p["du"], progress_bar=False, **kw)
    exp = m4q.QExperiment(p["plant_op0"][0], list(p["plant_ops"][0]))
    exp.set_noise(noise)
    (d1, _, c1) = run(exp)
    assert launches == [1]
    (d2, _, c2) = run(exp, exit_condition=lambda xn, x, u: False)
    assert launches == [1, 8]
    ob = m4q.MeasurementNoise(5e-3, seed=99, kind=kind)
    q = dict(p, batch=8, x0=np.repeat(p["x0"], 8, axis=0))          # member 7 of the oracle's ensemble: the same initial state
    (xo, uo), _, co = noisy_oracle_run(q, 7, ob)
    assert c1 == c2 == co == 0

    def rel(a, b):
        return np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert rel(d1[0], xo) <= 1e-8 and rel(d1[1], uo) <= 1e-8
    assert rel(d2[0], xo) <= 1e-8 and rel(d2[1], uo) <= 1e-8
    exp.set_noise(None)
    (d0, _, _) = run(exp)
    assert launches == [1, 8, 1] and np.abs(d0[0] - d1[0]).max() > 1e-4
    exp.set_sigma(5e-3)                                              # the reference's host noise: one launch per step, np.random
    np.random.seed(1)
    (d3, _, c3) = run(exp)
    assert launches == [1, 8, 1, 8] and c3 == 0 and np.abs(d3[0] - d0[0]).max() > 1e-4


# ---------------------------------------------------------------- 9. refusals of the C ABI against a live session
def test_capi_refusals_on_a_live_session():
    L = _lib.lib()
    dp = _lib._dp

    def rc(sess, mode, sigma, per=0, seed=1, base=0):
        a = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
        return L.m4q_session_set_noise(sess._h, mode, None if a is None else a.ctypes.data_as(dp), per, seed, base)

    p = kv.scenario(9, 2, 1, n_steps=4)
    cell = kv.LoopCell(9, 2, 1, kv.TILE, False, kv.HAMILTONIAN)
    sess = _open(cell, p)
    try:
        assert rc(sess, 3, [0.1]) == _lib.E_BADARG and rc(sess, -1, [0.1]) == _lib.E_BADARG
        assert rc(sess, _lib.NOISE_IID, None) == _lib.E_BADARG
        assert rc(sess, _lib.NOISE_IID, [-0.1]) == _lib.E_BADARG
        assert rc(sess, _lib.NOISE_HERMITIAN, [0.1, 0.1, float("nan"), 0.1, 0.1], per=1) == _lib.E_BADARG
        assert rc(sess, _lib.NOISE_IID, [float("inf")]) == _lib.E_BADARG
        assert sess.path_detail() == kv.TILE                                  # nothing was set
        assert rc(sess, _lib.NOISE_IID, [0.1]) == 0 and sess.path_detail() == kv.COMPLEX
        assert rc(sess, _lib.NOISE_HERMITIAN, [0.1]) == 0 and sess.path_detail() == kv.TILE     # before the first run: any change
        sess.run(0, 2)
        sess.sync()
        assert rc(sess, _lib.NOISE_IID, [0.1]) == _lib.E_BADARG                # the mode is fixed now
        assert b"cannot change" in L.m4q_last_error()
        assert rc(sess, 0, None) == _lib.E_BADARG
        assert rc(sess, _lib.NOISE_HERMITIAN, [0.2, 0.1, 0.3, 0.1, 0.2], per=1, seed=9, base=1 << 50) == 0      # the rest may change
        sess.run(2, 4)
        sess.sync()
        assert sess.path_detail() == kv.TILE
    finally:
        sess.close()
    quiet = _open(cell, p)
    try:
        quiet.run(0, 2)
        quiet.sync()
        assert rc(quiet, _lib.NOISE_HERMITIAN, [0.1]) == _lib.E_BADARG         # off is a mode too
        assert rc(quiet, 0, None) == 0
    finally:
        quiet.close()
    none = _open(kv.LoopCell(9, 2, 1, kv.COMPLEX, False, kv.NONE), p)
    try:
        assert rc(none, _lib.NOISE_IID, [0.1]) == _lib.E_BADARG and rc(none, _lib.NOISE_HERMITIAN, [0.1]) == _lib.E_BADARG
        assert rc(none, 0, None) == 0
        with pytest.raises(ValueError):
            none.set_noise(m4q.MeasurementNoise(0.1, 1))
    finally:
        none.close()
    ps = kv.process_scenario(1, 1, n_steps=4)
    proc = _open(kv.LoopCell(16, 1, 1, kv.COMPLEX, False, kv.PROCESS), ps)
    try:
        assert rc(proc, _lib.NOISE_HERMITIAN, [0.1]) == _lib.E_BADARG
        assert b"process" in L.m4q_last_error().lower()
        assert rc(proc, _lib.NOISE_IID, [0.1]) == 0
        with pytest.raises(ValueError):
            proc.set_noise(m4q.MeasurementNoise(0.1, 1, "hermitian"))
        with pytest.raises(TypeError):
            proc.set_noise(0.1)
    finally:
        proc.close()

"""QuadraticExit on the host (no device): the reference-form callables it stands for, the decisions of the goldens' own
conditions on their stored trajectories, the rejections the batched entry points raise before any device call, the fused-or-host
choice of mpc(), and the per-block slicing of mpc_batch_sharded."""
import os
import sys

import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from mpc4quantum_amd.mpc import _runs_fused, mpc_batch, open_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---------------------------------------------------------------- the callable
@pytest.mark.parametrize("state", ["prev", "next"])
@pytest.mark.parametrize("fires", ["below", "above"])
def test_call_equals_reference_form(state, fires):
    rng = np.random.default_rng(3)
    n = 9
    W, f = _rand(rng, n, n), _rand(rng, n)                     # not Hermitian: the real part is what counts
    qs = []
    for trial in range(200):
        xn, x = _rand(rng, n), _rand(rng, n)
        qs.append(((x - f).conj().T @ W @ (x - f)).real if state == "prev" else ((xn - f).conj().T @ W @ (xn - f)).real)
    for thr in (-1.0, 0.0, float(np.median(qs))):
        cond = m4q.QuadraticExit(W, f, thr, state=state, fires=fires)
        rng2 = np.random.default_rng(3)
        _rand(rng2, n, n), _rand(rng2, n)
        for trial in range(200):
            xn, x = _rand(rng2, n), _rand(rng2, n)
            p = x if state == "prev" else xn
            q = ((p - f).conj().T @ W @ (p - f)).real
            assert cond(xn, x, np.zeros(1)) == (q < thr if fires == "below" else q > thr)
    # abs(x_next[i]) > t, negative t included
    for t in (0.3, -0.5):
        W1 = np.zeros((n, n))
        W1[4, 4] = 1.0
        cond = m4q.QuadraticExit(W1, np.zeros(n), t * t if t >= 0 else -1.0, state="next", fires="above")
        for trial in range(100):
            xn = 0.4 * _rand(rng, n)
            assert cond(xn, None, None) == (abs(xn[4]) > t)


def test_per_member_call_and_block():
    rng = np.random.default_rng(5)
    n, B = 4, 6
    W, f, thr = np.identity(n), _rand(rng, B, n), np.arange(B, dtype=float)
    cond = m4q.QuadraticExit(W, f, thr)
    assert cond.members == B and cond.mode == _lib.EXIT_PREV | _lib.EXIT_BELOW
    with pytest.raises(ValueError):
        cond(f[0], f[0], None)                                    # which member?
    assert cond(None, f[2], None, member=2)                      # q = 0 < 2
    assert not cond(None, f[0], None, member=0)                  # q = 0, not < 0
    blk = cond.block(2, 5, B)
    assert np.array_equal(blk.target, f[2:5]) and np.array_equal(blk.thr, thr[2:5]) and blk.members == 3
    shared = m4q.QuadraticExit(W, f[0], 0.5, state="next", fires="above")
    assert shared.block(2, 5, B).members is None and shared.mode == _lib.EXIT_NEXT | _lib.EXIT_ABOVE


# ---------------------------------------------------------------- the goldens' own conditions
def test_synthesis_golden_decisions():
    g = np.load(os.path.join(GOLDEN, "synthesis.npz"))
    pf, Q = g["not_pf"], g["not_Q"]
    names = sorted({k[len("not_"):-len("_exit_thr")] for k in g.files if k.endswith("_exit_thr") and k.startswith("not_")})
    seen = 0
    for name in names:
        if not bool(g["not_%s_exit" % name]):
            continue
        thr, xs, code = float(g["not_%s_exit_thr" % name]), g["not_%s_xs" % name], int(g["not_%s_exit_code" % name])
        cond = m4q.QuadraticExit(Q, pf, thr, state="prev", fires="below")
        ref = lambda p2, p1, u1: ((p1 - pf).conj().T @ Q @ (p1 - pf)).real < thr      # noqa: E731
        for k in range(xs.shape[1] - 1):
            assert cond(xs[:, k + 1], xs[:, k], None) == ref(xs[:, k + 1], xs[:, k], None) == False     # noqa: E712
        # code 1: fired on the last stored state (the step it ended with, whose x_next was dropped)
        assert cond(None, xs[:, -1], None) == (code == 1) == ref(None, xs[:, -1], None)
        seen += 1
    assert seen >= 6


@pytest.mark.parametrize("name", ["qubit_o1_exit_step3", "qubit_o1_exit_step0"])
def test_mpc_loop_golden_decisions(name):
    g = np.load(os.path.join(GOLDEN, "mpc_loop.npz"))
    k = "loop_" + name + "_"
    i, t, xs = int(g[k + "exit_index"]), float(g[k + "exit_thr"]), g[k + "xs"]
    n = xs.shape[0]
    W = np.zeros((n, n))
    W[i, i] = 1.0
    cond = m4q.QuadraticExit(W, np.zeros(n), t * t if t >= 0 else -1.0, state="next", fires="above")
    ref = lambda xn, x, u: abs(xn[i]) > t      # noqa: E731
    for s in range(xs.shape[1]):
        assert cond(xs[:, s], None, None) == ref(xs[:, s], None, None)
        assert s == 0 or not ref(xs[:, s], None, None)            # (x_next of steps 0 .. done-1; the firing one is dropped)


# ---------------------------------------------------------------- rejections, before any device call
def test_shape_and_mode_rejections():
    n = 4
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros(n), 0.1, state="last")
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros(n), 0.1, fires="equal")
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.zeros((n, n + 1)), np.zeros(n), 0.1)
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros(n + 1), 0.1)
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros((3, n)), np.zeros(4))
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros(n), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros((3, n)), 0.1).check(4, n)
    with pytest.raises(ValueError):
        m4q.QuadraticExit(np.identity(n), np.zeros(n), 0.1).check(4, 9)


def _fail_session(*a, **k):
    raise AssertionError("a device session was opened")


def test_batch_entry_points_reject_before_the_device(monkeypatch):
    monkeypatch.setattr(sys.modules["mpc4quantum_amd.mpc"], "EnsembleSession", _fail_session)
    p = configs.build(2, batch=3, horizon=4, n_steps=2)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    args = (p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"], p["plant_ops"], p["Q"],
            p["R"], p["Qf"], p["sat"], p["du"])
    n = p["dim_x"]
    with pytest.raises(TypeError):
        mpc_batch(*args, exit_condition=lambda xn, x, u: False)
    with pytest.raises(TypeError):
        open_session(*args, exit_condition=lambda xn, x, u: False)
    with pytest.raises(ValueError):
        mpc_batch(*args, exit_condition=m4q.QuadraticExit(np.identity(n + 1), np.zeros(n + 1), 0.1))
    with pytest.raises(ValueError):
        mpc_batch(*args, exit_condition=m4q.QuadraticExit(np.identity(n), np.zeros((5, n)), 0.1))
    with pytest.raises(ValueError):
        mpc_batch(*args, plant_kind=_lib.PLANT_NONE, exit_condition=m4q.QuadraticExit(np.identity(n), np.zeros(n), 0.1))
    from mpc4quantum_amd.distributed import mpc_batch_sharded
    with pytest.raises(TypeError):                                # (transport=None: raised before RCCL is touched)
        mpc_batch_sharded(*args, exit_condition=lambda xn, x, u: False)
    with pytest.raises(ValueError):
        mpc_batch_sharded(*args, exit_condition=m4q.QuadraticExit(np.identity(n), np.zeros(n), np.zeros(7)))


def test_capi_set_exit_null_session():
    L = _lib.lib()
    one = np.zeros(2)
    rc = L.m4q_session_set_exit(None, _lib.EXIT_PREV | _lib.EXIT_BELOW, one.ctypes.data_as(_lib._dp), one.ctypes.data_as(_lib._dp),
                                0, one.ctypes.data_as(_lib._dp), 0)
    assert rc == _lib.E_BADARG


# ---------------------------------------------------------------- mpc(): fused or host
def test_mpc_fused_or_host_decision():
    n = 4
    qe = m4q.QuadraticExit(np.identity(n), np.zeros(n), 0.1)
    H = [np.diag([1.0, -1.0]).astype(complex), np.array([[0, 1], [1, 0]], dtype=complex)]
    native = m4q.QExperiment(H[0], H[1:])
    synth = m4q.QSynthesis(H[0], H[1:])

    class Lifted(m4q.QExperiment):
        def lift(self, x):
            return x

    assert _runs_fused(native, None, False) and _runs_fused(native, qe, False) and _runs_fused(synth, qe, False)
    assert not _runs_fused(native, lambda xn, x, u: False, False)           # a plain callable keeps the host path
    assert not _runs_fused(synth, lambda xn, x, u: False, False)
    assert not _runs_fused(native, qe, True)                                 # streaming
    assert not _runs_fused(Lifted(H[0], H[1:]), qe, False)                   # a lift of its own: host plant


# ---------------------------------------------------------------- mpc_batch_sharded slicing (gloo host transport)
def _echo_solver(x0, models, dim_u, order, X_targ, U_targ, clock, op0, ops, Q, R, Qf, sat, du, exit_condition=None, **kw):
    """Returns its block's exit condition as results: xs[:, :, 0] the targets, steps_done the thresholds."""
    k, n, ns = len(x0), x0.shape[1], clock.n_steps
    xs = np.zeros((k, n, ns + 1), dtype=complex)
    xs[:, :, 0] = exit_condition.target
    return {"xs": xs, "us": np.zeros((k, dim_u, ns)), "exit_codes": np.ones(k, dtype=np.int32),
            "steps_done": exit_condition.thr.astype(np.int32), "qp_solves": np.zeros((k, ns), dtype=np.int32)}


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from mpc4quantum_amd.distributed import mpc_batch_sharded
    from gloo_transport import GlooTransport
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p = configs.build(2, batch=5, horizon=6, n_steps=4)
    clock = m4q.StepClock(p["dt"], p["horizon"], p["n_steps"])
    n = p["dim_x"]
    target = np.arange(5 * n).reshape(5, n) * (1 + 1j)
    cond = m4q.QuadraticExit(np.identity(n), target, np.arange(5) + 1.0, state="next", fires="above")
    res = mpc_batch_sharded(p["x0"], p["models"], p["dim_u"], p["order"], p["X_targ"], p["U_targ"], clock, p["plant_op0"],
                            p["plant_ops"], p["Q"], p["R"], p["Qf"], p["sat"], p["du"], solver=_echo_solver,
                            transport=GlooTransport(), exit_condition=cond)
    if rank == 0:
        np.savez(out_path, **res)
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_sharded_slices_per_member_targets_and_thresholds(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "gathered.npz")
    port = 29500 + (os.getpid() % 2000) + 13
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    got = np.load(out)
    n = got["xs"].shape[1]
    assert np.array_equal(got["xs"][:, :, 0], np.arange(5 * n).reshape(5, n) * (1 + 1j))
    assert np.array_equal(got["steps_done"], np.arange(5) + 1)

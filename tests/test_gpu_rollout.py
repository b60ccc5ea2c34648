"""The open-loop rollouts on the device (plant_rollout_kernel, model_rollout_kernel) against independent references: the oracle's
plant steps chained (SciPy expm), a few lines of expm for the process plant, OracleDMDc.predict with OracleWrapModel's lifted
controls for the models.  Tolerance of DESIGN section 3: 1e-10 max(1, |x|_inf).  Shapes are the smallest that can go wrong: B = 5
(a ragged quad) and B = 1, N in {1, 7, 33}; one case with 4,098 quads, one more than the grid the launch is capped at."""
import numpy as np
import pytest

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib, configs
from oracle import m4q_oracle as orc
from tests import kernel_variants as kv

pytestmark = pytest.mark.gpu

TOL = 1e-10


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


def _herm(rng, d):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return 0.5 * (M + M.conj().T)


def _densities(rng, d, B):
    out = []
    for _ in range(B):
        M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        rho = M @ M.conj().T
        out.append((rho / np.trace(rho).real).reshape(-1))
    return np.ascontiguousarray(out)


def _process_vectors(rng, B):
    from scipy.linalg import expm
    out = []
    for _ in range(B):
        U = expm(-1j * _herm(rng, 2))
        out.append(np.kron(U, U.conj()).reshape(-1))
    return np.ascontiguousarray(out)


def _process_step(P, u, H0, Hs, dt):
    """(V (x) V^*) M on the process vector P = vec_r(M), V = expm(-i dt (H0 + sum_k u_k H_k))."""
    from scipy.linalg import expm
    H = H0 + sum(float(uk) * h for uk, h in zip(u, Hs))
    V = expm(-1j * dt * H)
    return (np.kron(V, V.conj()) @ np.reshape(P, (4, 4))).reshape(-1)


# ---------------------------------------------------------------- the plant cases
class Case:
    """One shape and plant kind: the operators and bound of its configuration, the reference step, and (generator) the
    experiment whose operators() the rollout goes through."""

    def __init__(self, name):
        self.name = name
        self.exp = None
        if name == "4-1-hamiltonian":
            p = configs.build(1)
        elif name in ("9-2-hamiltonian", "9-2-generator"):
            p = configs.build(3, batch=1)
        elif name == "16-3-hamiltonian":
            p = configs.build(4, batch=1)
        elif name == "16-2-hamiltonian":                         # the plant-only shape: config 4's pair under its two sigma_y drives
            p = configs.build(4, batch=1)
            p["plant_ops"] = p["plant_ops"][:, :2]
        else:
            assert name == "16-1-process"
            p = configs.synthesis(1)
            p["plant_op0"] = 0.15 * configs.SZ[None]
        self.dt, self.sat = p["dt"], p["sat"]
        self.op0, self.ops = np.array(p["plant_op0"][0]), np.array(p["plant_ops"][0])
        self.kind, self.step, self.bound = _lib.PLANT_HAMILTONIAN, orc.plant_step, 1e-12
        self.d = self.op0.shape[0]
        self.n = self.d ** 2
        if name == "9-2-generator":
            a = np.diag(np.sqrt(np.arange(1, 3)), 1).astype(complex)
            self.exp = m4q.QExperiment(self.op0, list(self.ops))
            self.exp.set("c_ops", [0.2 * a])                     # one collapse operator: operators() are Lindblad generators
            self.op0, self.ops = self.exp.operators()
            assert self.exp.plant_kind == _lib.PLANT_GENERATOR and self.op0.shape == (9, 9)
            self.kind, self.step, self.bound = _lib.PLANT_GENERATOR, orc.plant_step_generator, 1e-11
        elif name == "16-1-process":
            self.kind, self.step, self.n = _lib.PLANT_PROCESS, _process_step, 16
        self.m = self.ops.shape[0]

    def states(self, rng, B):
        return _process_vectors(rng, B) if self.kind == _lib.PLANT_PROCESS else _densities(rng, self.d, B)

    def member_ops(self, rng, B):
        """Per-member operators: the configuration's, detuned and rescaled member by member (a valid plant of the same kind)."""
        if self.kind == _lib.PLANT_GENERATOR:
            op0 = np.stack([self.op0 + m4q.liouvillian(0.1 * _herm(rng, self.d)) for _ in range(B)])
        else:
            op0 = np.stack([(1 + 0.05 * rng.standard_normal()) * self.op0 + 0.1 * _herm(rng, self.d) for _ in range(B)])
        ops = np.stack([(1 + 0.02 * rng.standard_normal()) * self.ops for _ in range(B)])
        return op0, ops


CASES = {name: None for name in ("4-1-hamiltonian", "9-2-hamiltonian", "9-2-generator", "16-3-hamiltonian", "16-2-hamiltonian",
                                 "16-1-process")}


def case(name):
    if CASES[name] is None:
        CASES[name] = Case(name)
    return CASES[name]


def _grid(rng, N, dt):
    """A non-uniform time grid of N intervals around dt."""
    return np.concatenate([[0.0], np.cumsum(dt * rng.uniform(0.4, 1.6, N))])


def _chain(c, x0, u, op0, ops, dts):
    """The reference: the oracle's held-control step, member by member and interval by interval.  u [B, N, m], op0 / ops [B, ...]."""
    B, N = u.shape[:2]
    xs = np.empty((B, N + 1, c.n), dtype=complex)
    for b in range(B):
        x = xs[b, 0] = x0[b]
        for t in range(N):
            x = xs[b, t + 1] = c.step(x, u[b, t], op0[b], list(ops[b]), dts[t])
    return xs


# variant: what is shared by the ensemble and what is the member's own
#   shared  one operator set, one control sequence, u_scale, non-uniform grid
#   per     per-member operators and control sequences, scalar dt
#   mixed   per-member drift operator beside shared control operators, one sequence, u_scale, non-uniform grid (a robustness landscape)
RUNS = [("shared", 5, 33), ("per", 5, 7), ("mixed", 5, 7), ("per", 1, 1), ("shared", 1, 7), ("mixed", 5, 1)]


@pytest.mark.parametrize("variant,B,N", RUNS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(CASES))
def test_plant_rollout_against_the_reference_chain(name, variant, B, N):
    c = case(name)
    rng = np.random.default_rng(7000 + 13 * list(CASES).index(name) + 101 * B + N)
    x0 = c.states(rng, B)
    m = c.m
    op0_b, ops_b = c.member_ops(rng, B)
    if variant == "per":
        u = rng.uniform(-c.sat, c.sat, (B, N, m))
        ts, sc = np.arange(N + 1) * c.dt, None
        op0, ops = op0_b, (None if c.exp else ops_b)
        ref = _chain(c, x0, u, op0_b, np.stack([c.ops] * B) if c.exp else ops_b, np.full(N, c.dt))
    else:
        u = rng.uniform(-c.sat, c.sat, (N, m))
        ts, sc = _grid(rng, N, c.dt), 1 + 0.1 * rng.standard_normal((B, m))
        op0, ops = (op0_b, None) if variant == "mixed" else (None, None)
        ref = _chain(c, x0, sc[:, None, :] * u[None], op0_b if variant == "mixed" else np.stack([c.op0] * B), np.stack([c.ops] * B),
                     np.diff(ts))
    if c.exp is not None:
        # the experiment's own entry point, controls as simulate() takes them: (m, len(ts)), (B, m, len(ts)); the last column is unused
        us = np.concatenate([np.moveaxis(u, -1, -2), np.zeros(u.shape[:-2] + (m, 1))], axis=-1)
        out = c.exp.simulate_batch(x0, ts, us, op0=op0, u_scale=sc)
    else:
        out = m4q.plant_rollout_batch(x0, u, c.op0 if op0 is None else op0, c.ops if ops is None else ops,
                                      c.dt if variant == "per" else ts, c.kind, u_scale=sc)
    xs = out["xs"]
    assert set(out) == {"xs"} and xs.shape == (B, N + 1, c.n)
    assert np.array_equal(xs[:, 0].view(np.float64), x0.view(np.float64))                # column 0 is x0 bit for bit
    err = np.abs(xs - ref).max()
    print("%s %s B=%d N=%d: max|dx| = %.2e" % (name, variant, B, N, err))
    assert err <= TOL * max(1.0, np.abs(ref).max())
    last = (c.exp.simulate_batch(x0, ts, us, op0=op0, u_scale=sc, keep="last") if c.exp is not None else
            m4q.plant_rollout_batch(x0, u, c.op0 if op0 is None else op0, c.ops if ops is None else ops,
                                    c.dt if variant == "per" else ts, c.kind, u_scale=sc, keep="last"))
    assert np.array_equal(last["xs"], xs[:, N])


@pytest.mark.parametrize("name", list(CASES))
def test_rollout_step_by_step_against_plant_step_batch(name, record_property):
    """Column t of a rollout and u_t through m4q_plant_step_batch give column t + 1, to the bound tests/test_gpu_variant_matrix.py
    holds one step to against the oracle (1e-12 Hamiltonian / process, 1e-11 generator).  The two kernels inline one device
    function: identical bits are expected, not promised - the maximum and whether every bit agreed are recorded."""
    c = case(name)
    B, N = 5, 7
    rng = np.random.default_rng(7500 + list(CASES).index(name))
    x0 = c.states(rng, B)
    op0, ops = c.member_ops(rng, B)
    u = rng.uniform(-c.sat, c.sat, (B, N, c.m))
    ts = _grid(rng, N, c.dt)
    xs = m4q.plant_rollout_batch(x0, u, op0, ops, ts, c.kind)["xs"]
    worst, same = 0.0, True
    for t in range(N):
        nxt = m4q.plant_step_batch(xs[:, t], u[:, t], op0, ops, ts[t + 1] - ts[t], c.kind)
        worst = max(worst, rel(xs[:, t + 1], nxt))
        same = same and np.array_equal(xs[:, t + 1].view(np.float64), nxt.view(np.float64))
    record_property("max_rel_diff", worst)
    record_property("bit_identical", same)
    print("%s: rollout against %d single steps: max rel diff %.3e, bit identical: %s" % (name, N, worst, same))
    assert worst <= c.bound


def _figure(xs, W, f):
    d = xs - f[:, None, :]
    return np.einsum('btj,jk,btk->bt', d.conj(), W, d).real, np.abs(d).max()


def _options_agree(run, x0, u, sc, W, f):
    """run(us, u_scale, keep, figure) -> dict.  The checks of every option against the full run, bit for bit."""
    B, N = x0.shape[0], u.shape[0]
    full = run(u, sc, "all", "all")
    xs, q = full["xs"], full["q"]
    assert xs.shape == (B, N + 1, x0.shape[1]) and q.shape == (B, N + 1)
    assert np.array_equal(xs[:, 0].view(np.float64), x0.view(np.float64))
    last = run(u, sc, "last", "last")
    assert np.array_equal(last["xs"], xs[:, N]) and np.array_equal(last["q"], q[:, N])
    fig = run(u, sc, "none", "all")
    assert set(fig) == {"q"} and np.array_equal(fig["q"], q)
    fig = run(u, sc, "none", "last")
    assert set(fig) == {"q"} and np.array_equal(fig["q"], q[:, N])
    mixed = run(u, sc, "last", "all")
    assert np.array_equal(mixed["xs"], xs[:, N]) and np.array_equal(mixed["q"], q)
    tiled = run(np.tile(u[None], (B, 1, 1)), sc, "all", "all")
    assert np.array_equal(tiled["xs"], xs) and np.array_equal(tiled["q"], q)
    pre = run(sc[:, None, :] * u[None], None, "all", "all")
    assert np.array_equal(pre["xs"], xs) and np.array_equal(pre["q"], q)
    # the figure against NumPy on the returned states: a 16-term fp64 sum per row
    q_np, dmax = _figure(xs, W, f)
    tol = 1e-12 * max(1.0, np.abs(W).sum() * dmax ** 2)
    print("figure: max|dq| = %.2e (tolerance %.2e), column 0: %.2e" % (np.abs(q - q_np).max(), tol, np.abs(q[:, 0] - q_np[:, 0]).max()))
    assert np.abs(q - q_np).max() <= tol
    assert np.abs(q[:, 0] - q_np[:, 0]).max() <= tol and np.abs(q[:, 0]).min() > 0       # (column 0: x0 itself against f)


def _weights(rng, n, B):
    """A non-Hermitian W and per-member targets."""
    W = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    f = rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n))
    assert np.abs(W - W.conj().T).max() > 0.1
    return W, 0.3 * f


def test_plant_rollout_options_agree_bitwise():
    c = case("9-2-hamiltonian")
    B, N = 5, 7
    rng = np.random.default_rng(7600)
    x0 = c.states(rng, B)
    op0, _ = c.member_ops(rng, B)
    u = rng.uniform(-c.sat, c.sat, (N, c.m))
    sc = 1 + 0.1 * rng.standard_normal((B, c.m))
    W, f = _weights(rng, c.n, B)
    ts = _grid(rng, N, c.dt)
    _options_agree(lambda us, s, keep, figure: m4q.plant_rollout_batch(x0, us, op0, c.ops, ts, c.kind, u_scale=s, W=W, target=f, keep=keep,
                                                                       figure=figure), x0, u, sc, W, f)
    # one target for the ensemble equals the same target given per member
    one = m4q.plant_rollout_batch(x0, u, op0, c.ops, ts, c.kind, W=W, target=f[0], keep="none", figure="all")["q"]
    per = m4q.plant_rollout_batch(x0, u, op0, c.ops, ts, c.kind, W=W, target=np.tile(f[:1], (B, 1)), keep="none", figure="all")["q"]
    assert np.array_equal(one, per)


def test_model_rollout_options_agree_bitwise():
    p = kv.scenario(9, 2, 1)
    B, N = 5, 7
    rng = np.random.default_rng(7601)
    sat = p["sat"] / kv.TUNING[(9, 2)][1]
    u = rng.uniform(-sat, sat, (N, 2))
    sc = 1 + 0.1 * rng.standard_normal((B, 2))
    W, f = _weights(rng, 9, B)
    x0 = np.ascontiguousarray(p["x0"])
    _options_agree(lambda us, s, keep, figure: m4q.model_rollout_batch(x0, us, p["models"], 1, u_scale=s, W=W, target=f, keep=keep,
                                                                       figure=figure), x0, u, sc, W, f)


# ---------------------------------------------------------------- place and neighbours
PICK = (0, 16383, 16384, 16388)


def _big(rng):
    B, N = 16389, 3                        # 4,098 quads - one more than the 4,096 workgroups of the launch -, the last one ragged
    c = case("4-1-hamiltonian")
    x0 = np.tile(c.states(rng, 64), (B // 64 + 1, 1))[:B] * (1 + 1e-3 * rng.standard_normal((B, 1)))
    u = rng.uniform(-c.sat, c.sat, (B, N, 1))
    sc = 1 + 0.1 * rng.standard_normal((B, 1))
    W, f = _weights(rng, 4, B)
    return c, B, N, np.ascontiguousarray(x0), u, sc, W, f


def _same_alone(run_all, run_one):
    full = run_all()
    assert np.isfinite(full["xs"]).all() and np.isfinite(full["q"]).all()
    for b in PICK:
        one = run_one(b)
        assert np.array_equal(one["xs"][0].view(np.float64), full["xs"][b].view(np.float64)), b
        assert np.array_equal(one["q"][0], full["q"][b]), b
    assert len({full["xs"][b].tobytes() for b in PICK}) == len(PICK)                      # (the members do differ)


def test_plant_rollout_member_does_not_depend_on_its_place():
    rng = np.random.default_rng(7700)
    c, B, N, x0, u, sc, W, f = _big(rng)
    op0 = (1 + 0.05 * rng.standard_normal((B, 1, 1))) * c.op0[None]
    ts = _grid(rng, N, c.dt)
    _same_alone(lambda: m4q.plant_rollout_batch(x0, u, op0, c.ops, ts, c.kind, u_scale=sc, W=W, target=f, figure="all"),
                lambda b: m4q.plant_rollout_batch(x0[b:b + 1], u[b:b + 1], op0[b], c.ops, ts, c.kind, u_scale=sc[b:b + 1], W=W,
                                                  target=f[b:b + 1], figure="all"))


def test_model_rollout_member_does_not_depend_on_its_place():
    rng = np.random.default_rng(7701)
    c, B, N, x0, u, sc, W, f = _big(rng)
    base = kv.scenario(4, 1, 1)["models"][0]
    models = base[None] * (1 + 0.01 * rng.standard_normal((B, 1, 1)))
    _same_alone(lambda: m4q.model_rollout_batch(x0, u, models, 1, u_scale=sc, W=W, target=f, figure="all"),
                lambda b: m4q.model_rollout_batch(x0[b:b + 1], u[b:b + 1], models[b], 1, u_scale=sc[b:b + 1], W=W, target=f[b:b + 1],
                                                  figure="all"))


# ---------------------------------------------------------------- models
MODEL_SHAPES = [(4, 1, 1), (4, 1, 2), (9, 2, 1), (9, 2, 2), (16, 3, 1), (8, 2, 1), (16, 1, 4)]


def _model_chain(model, m, order, x0, u):
    """OracleDMDc.predict along u [N, m] with OracleWrapModel's lifted controls (mpc.py:267's call shape)."""
    n = x0.shape[0]
    wm = orc.OracleWrapModel(model[:, :n], model[:, n:], m, order)
    dm = orc.OracleDMDc(n, n, model.shape[1] - n, model)
    xs = [x0]
    for t in range(u.shape[0]):
        x = xs[-1].reshape(-1, 1)
        xs.append(dm.predict(x, orc.krtimes(wm.lift_u(u[t]), x)).reshape(-1))
    return np.array(xs)


@pytest.mark.parametrize("per_member", [False, True], ids=["shared", "per-member"])
@pytest.mark.parametrize("shape", MODEL_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_model_rollout_against_the_oracle(shape, per_member):
    n, m, order = shape
    p = kv.scenario(n, m, order)
    B, N = 5, 33
    rng = np.random.default_rng(7800 + 100 * n + 10 * m + order + (1000 if per_member else 0))
    sat = p["sat"] / kv.TUNING[(n, m)][1]                      # the configuration's own bound: saturating random controls
    x0 = np.ascontiguousarray(p["x0"])
    assert p["models"].shape[0] == B
    if per_member:
        u = rng.uniform(-sat, sat, (B, N, m))
        models = p["models"]
        ref = np.stack([_model_chain(models[b], m, order, x0[b], u[b]) for b in range(B)])
    else:
        u = rng.uniform(-sat, sat, (N, m))
        models = p["models"][0]
        ref = np.stack([_model_chain(models, m, order, x0[b], u) for b in range(B)])
    out = m4q.model_rollout_batch(x0, u, models, order)
    xs = out["xs"]
    assert set(out) == {"xs"} and xs.shape == (B, N + 1, n)
    assert np.array_equal(xs[:, 0].view(np.float64), x0.view(np.float64))
    err = np.abs(xs - ref).max()
    print("model (%d, %d, %d) %s: max|x| = %.2e, max|dx| = %.2e" % (n, m, order, "per-member" if per_member else "shared",
                                                                   np.abs(ref).max(), err))
    assert err <= TOL * max(1.0, np.abs(ref).max())
    one = m4q.model_rollout_batch(x0[:1], u[0] if per_member else u, models[0] if per_member else models, order, keep="last")["xs"]
    assert np.array_equal(one[0], xs[0, N])                                               # B = 1, and N = 33 in one piece


@pytest.mark.parametrize("N", [1, 7])
def test_model_rollout_short_sequences(N):
    p = kv.scenario(4, 1, 2)
    rng = np.random.default_rng(7900 + N)
    u = rng.uniform(-1, 1, (1, N, 1))
    xs = m4q.model_rollout_batch(p["x0"][:1], u, p["models"][:1], 2)["xs"]
    ref = _model_chain(p["models"][0], 1, 2, p["x0"][0], u[0])
    assert xs.shape == (1, N + 1, 4) and np.abs(xs[0] - ref).max() <= TOL * max(1.0, np.abs(ref).max())


# ---------------------------------------------------------------- the experiments' entry points
def test_simulate_batch_follows_simulate():
    """simulate_batch of the three device plants against their own simulate(), member by member (ensemble axis first there,
    state axis first here), to the one-step bounds; simulate() and the experiment's record of its last run are untouched."""
    rng = np.random.default_rng(8000)
    ts = np.array([0.0, 0.2, 0.5, 0.55])
    for exp, states, m, bound in ((m4q.QExperiment(case("9-2-hamiltonian").op0, list(case("9-2-hamiltonian").ops)), _densities(rng, 3, 3), 2, 1e-12),
                                  (m4q.LExperiment(case("9-2-generator").op0, list(case("9-2-generator").ops)), _densities(rng, 3, 3), 2, 1e-11),
                                  (m4q.QSynthesis(0.15 * configs.SZ, [0.5 * configs.SX]), _process_vectors(rng, 3), 1, 1e-12)):
        us = rng.uniform(-1, 1, (m, len(ts)))
        out = exp.simulate_batch(states, ts, us)
        assert exp.xs is None and exp.ts is None
        for b in range(3):
            assert rel(out["xs"][b].T, exp.simulate(states[b], ts, us)) <= bound
        fn = exp.simulate_batch(states, ts, lambda t: us[:, int(np.searchsorted(ts, t))])
        assert np.array_equal(fn["xs"], out["xs"])

"""What the tests of the rollout gradients share (tests/test_grad_host.py, tests/test_gpu_grad.py): the plant and model cases, seeded
inputs, and independent forward chains - the oracle's plant step, a few lines of expm for the process plant, OracleDMDc.predict."""
import numpy as np

from mpc4quantum_amd import _lib, configs
from mpc4quantum_amd.configs import I2, SX, SY, SZ
from mpc4quantum_amd.vectorize import discretize_homogeneous, liouvillian
from oracle import m4q_oracle as orc


def _herm(rng, d):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return 0.5 * (M + M.conj().T)


def _process_step(P, u, H0, Hs, dt):
    """(V (x) V^*) M on the process vector P = vec_r(M), V = expm(-i dt (H0 + sum_k u_k H_k)) (tests/test_gpu_rollout.py, restated)."""
    from scipy.linalg import expm
    H = H0 + sum(float(uk) * h for uk, h in zip(u, Hs))
    V = expm(-1j * dt * H)
    return (np.kron(V, V.conj()) @ np.reshape(P, (4, 4))).reshape(-1)


class PlantCase:
    """One plant shape: (dim_x, dim_u), the plant kind, the operators, step and bound of its configuration."""

    def __init__(self, name):
        self.name = name
        self.kind, self.step = _lib.PLANT_HAMILTONIAN, orc.plant_step
        if name == "4-1":
            p = configs.build(1)
            op0, ops, self.dt, self.sat = p["plant_op0"][0], p["plant_ops"][0], p["dt"], p["sat"]
        elif name == "4-2":
            op0, ops, self.dt, self.sat = 0.15 * SZ, np.stack([0.5 * SX, 0.5 * SY]), 0.5, 2 * np.pi * 0.08
        elif name == "9-2":
            p = configs.build(3, batch=1)
            op0, ops, self.dt, self.sat = p["plant_op0"][0], p["plant_ops"][0], p["dt"], p["sat"]
        elif name in ("16-3", "16-2", "16-1"):                    # config 4's pair under its three, two (plant-only shape) or one drive
            p = configs.build(4, batch=1)
            op0, ops, self.dt, self.sat = p["plant_op0"][0], p["plant_ops"][0][:int(name[-1])], p["dt"], p["sat"]
        else:
            assert name in ("16-1-process", "16-2-process", "16-3-process")
            p = configs.synthesis(1)
            op0, ops, self.dt, self.sat = 0.15 * SZ, p["plant_ops"][0], p["dt"], p["sat"]
            if name != "16-1-process":                            # two or three drives, as kernel_variants.process_scenario(nu=3)
                ops = np.stack([0.5 * SX, 0.5 * SY, 0.5 * SZ])[:int(name[3])]
            self.kind, self.step = _lib.PLANT_PROCESS, _process_step
        self.op0, self.ops = np.array(op0, dtype=complex), np.array(ops, dtype=complex)
        self.d, self.m = self.op0.shape[0], self.ops.shape[0]
        self.n = self.d ** 4 if self.kind == _lib.PLANT_PROCESS else self.d ** 2

    def states(self, rng, B):
        from scipy.linalg import expm
        out = []
        for _ in range(B):
            if self.kind == _lib.PLANT_PROCESS:
                U = expm(-1j * _herm(rng, 2))
                out.append(np.kron(U, U.conj()).reshape(-1))
            else:
                M = rng.standard_normal((self.d, self.d)) + 1j * rng.standard_normal((self.d, self.d))
                rho = M @ M.conj().T
                out.append((rho / np.trace(rho).real).reshape(-1))
        return np.ascontiguousarray(out)

    def member_ops(self, rng, B):
        """Per-member operators: the configuration's, detuned and rescaled member by member."""
        op0 = np.stack([(1 + 0.05 * rng.standard_normal()) * self.op0 + 0.1 * _herm(rng, self.d) for _ in range(B)])
        ops = np.stack([(1 + 0.02 * rng.standard_normal()) * self.ops for _ in range(B)])
        return op0, ops


PLANT_NAMES = ("4-1", "4-2", "9-2", "16-3", "16-1", "16-1-process")          # the six cases of the host check
_PLANTS = {}


def plant_case(name):
    if name not in _PLANTS:
        _PLANTS[name] = PlantCase(name)
    return _PLANTS[name]


def weights_and_targets(rng, n, B):
    """A non-Hermitian W and per-member targets."""
    W = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    f = 0.3 * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    assert np.abs(W - W.conj().T).max() > 0.1
    return W, f


def grid(rng, N, dt):
    """A non-uniform time grid of N intervals around dt."""
    return np.concatenate([[0.0], np.cumsum(dt * rng.uniform(0.4, 1.6, N))])


def figures(xs, W, f):
    """q [.., N + 1] of states xs [.., N + 1, n] against f [.., n]."""
    d = xs - f[..., None, :]
    return np.einsum('...tj,jk,...tk->...t', d.conj(), W, d).real


def plant_chain(c, x0, v, op0, ops, dts):
    """One member's states [N + 1, n] under the controls v [N, m] it sees: the independent step, interval by interval."""
    xs = [np.asarray(x0)]
    for t in range(v.shape[0]):
        xs.append(c.step(xs[-1], v[t], op0, list(ops), dts[t]))
    return np.array(xs)


# ---------------------------------------------------------------- models
MODEL_SHAPES = [(4, 1, 1), (4, 1, 2), (9, 2, 2), (8, 2, 1), (16, 1, 4)]


def model_case(n, m, order, B, seed):
    """Per-member models [B, n, n (1 + P)] from discretize_homogeneous of detuned generators, states and a control bound."""
    rng = np.random.default_rng(seed)
    if (n, m) == (4, 1):
        H0, Hk, dt, sat = 0.15 * SZ, [0.5 * SX], 0.5, 2 * np.pi * 0.1
    elif (n, m) == (9, 2):
        p = configs.build(3, batch=1, drift_scale=0.125)
        H0, Hk, dt, sat = p["plant_op0"][0], list(p["plant_ops"][0]), p["dt"], p["sat"]
    elif (n, m) == (16, 1):
        H0, Hk, dt, sat = np.kron(SZ, SZ), [np.kron(SY, I2)], 0.25, 2 * np.pi * 0.05
    else:
        assert (n, m) == (8, 2)
        H0 = Hk = None
        dt, sat = 0.5, 2 * np.pi * 0.1
    models, x0 = [], []
    for _ in range(B):
        s = 1 + 0.05 * rng.standard_normal()
        if H0 is None:           # the reduced crosstalk model: two qubit states side by side
            z = np.zeros((4, 4))
            gens = [np.block([[liouvillian(0.05 * s * SZ), z], [z, liouvillian(-0.05 * s * SZ)]]),
                    np.block([[liouvillian(SX), z], [z, z]]), np.block([[z, z], [z, liouvillian(SY)]])]
            d, parts = 2, 2
        else:
            gens = [s * liouvillian(H0)] + [liouvillian(h) for h in Hk]
            d, parts = H0.shape[0], 1
        models.append(discretize_homogeneous(gens, dt, order))
        st = []
        for _ in range(parts):
            M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
            rho = M @ M.conj().T
            st.append((rho / np.trace(rho).real).reshape(-1))
        x0.append(np.concatenate(st))
    return np.ascontiguousarray(models), np.ascontiguousarray(x0), sat, rng


def model_chain(model, m, order, x0, v):
    """OracleDMDc.predict along v [N, m] with OracleWrapModel's lifted controls."""
    n = x0.shape[0]
    wm = orc.OracleWrapModel(model[:, :n], model[:, n:], m, order)
    dm = orc.OracleDMDc(n, n, model.shape[1] - n, model)
    xs = [x0]
    for t in range(v.shape[0]):
        x = xs[-1].reshape(-1, 1)
        xs.append(dm.predict(x, orc.krtimes(wm.lift_u(v[t]), x)).reshape(-1))
    return np.array(xs)

"""What the tests of the plant-parameter gradient and of the calibration share (tests/test_plant_param_host.py,
tests/test_gpu_plant_param.py): the directions of each plant case, seeded inputs, and the calibration's case set."""
import numpy as np

import mpc4quantum_amd as m4q
from mpc4quantum_amd import _lib
from mpc4quantum_amd.plant_param import max_directions
from tests import grad_cases as gc
from tests import kernel_variants as kv


def _herm(rng, d):
    M = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    return 0.5 * (M + M.conj().T)


def physical_directions(d):
    """Detuning (the number operator) and anharmonicity (n (n - 1) / 2) of a d-level oscillator: [2, d, d]."""
    lv = np.arange(d, dtype=float)
    return np.stack([np.diag(lv), np.diag(0.5 * lv * (lv - 1))]).astype(complex)


def directions(rng, d, p, B=None):
    """p Hermitian directions [p, d, d]: the two physical ones first, random ones after; B: per-member [B, p, d, d], each member's own
    mix of them."""
    base = list(physical_directions(d))[:p] + [_herm(rng, d) for _ in range(max(0, p - 2))]
    base = np.stack(base[:p])
    if B is None:
        return base
    return np.stack([(1 + 0.2 * rng.standard_normal((p, 1, 1))) * base + 0.1 * np.stack([_herm(rng, d) for _ in range(p)]) for _ in range(B)])


def data_for(rng, c, B, N, per=True):
    """A 'measured' trajectory that is no rollout of the plant: [B, N + 1, n], or one [N + 1, n] shared by the ensemble."""
    y = 0.3 * (rng.standard_normal((B if per else 1, N + 1, c.n)) + 1j * rng.standard_normal((B if per else 1, N + 1, c.n)))
    return y if per else y[0]


def inputs(name, variant, B, N, p, seed):
    """One seeded call: (case, args, kwargs) of plant_param_grad_reference / plant_rollout_param_grad_batch.
    variant "shared": one operator set, one control sequence, shared dirs and data, u_scale, a non-uniform grid, col_w with zeros;
    variant "per": per-member operators, sequences, dirs and data, no u_scale, a scalar dt, default col_w."""
    c = gc.plant_case(name)
    rng = np.random.default_rng(seed)
    x0 = c.states(rng, B)
    W, _ = gc.weights_and_targets(rng, c.n, B)
    if variant == "per":
        op0, ops = c.member_ops(rng, B)
        u, ts, sc, cw = rng.uniform(-c.sat, c.sat, (B, N, c.m)), c.dt, None, None
        dirs, data = directions(rng, c.d, p, B), data_for(rng, c, B, N, True)
    else:
        op0, ops = c.op0, c.ops
        u, ts, sc = rng.uniform(-c.sat, c.sat, (N, c.m)), gc.grid(rng, N, c.dt), 1 + 0.1 * rng.standard_normal((B, c.m))
        cw = rng.uniform(0.5, 1.5, N + 1)
        cw[::3] = 0.0                                   # sparse measurement: columns 0, 3, 6 are not measured
        if N == 1:
            cw[1] = 1.0
        dirs, data = directions(rng, c.d, p), data_for(rng, c, B, N, False)
    return c, (x0, u, op0, ops, dirs, ts, W, data), dict(kind=c.kind, u_scale=sc, col_w=cw)


def p_max(name, scale_grad=False):
    c = gc.plant_case(name)
    return max_directions(c.d) - (c.m if scale_grad else 0)


def live_directions(rng, d, p, B=None):
    """directions(), with every direction that is the zero matrix (the anharmonicity of a two-level system: n (n - 1) / 2 = 0 at
    d = 2) replaced by one more random Hermitian draw: no column of the gradient is 0 by construction."""
    dirs = np.array(directions(rng, d, p, B))
    for j in range(p):
        if not dirs[..., j, :, :].any():
            dirs[..., j, :, :] = _herm(rng, d)
    return dirs


# ---------------------------------------------------------------- the direction-count matrix
# every (cell, PT) of kernel_variants.param_cells() at both splits of PT and in both layouts: B = 5 (a ragged quad), N = 2 (one step
# with a next step to prefetch, one without)
MATRIX_B, MATRIX_N = 5, 2
# A case whose reference fails the preconditions of tests/test_plant_param_host.py (a column of the gradient that is all but 0, two
# columns all but equal) draws again: {case id: draws skipped}.  None does.
MATRIX_RESEED = {}


def cell_name(nx, nu, kind):
    return "%d-%d%s" % (nx, nu, "-process" if kind == kv.PROCESS else "")


def matrix_cases():
    """[(name, PT, p, scale_grad, variant)]: (p = PT, no gains) and, where PT - m >= 1, (p = PT - m, the m gains)."""
    out = []
    for nx, nu, kind, pt in kv.param_cells():
        for p, sg in [(pt, False)] + ([(pt - nu, True)] if pt - nu >= 1 else []):
            out += [(cell_name(nx, nu, kind), pt, p, sg, variant) for variant in ("shared", "per")]
    return out


def matrix_id(case):
    name, pt, p, sg, variant = case
    return "%s-PT%d-p%d%s-%s" % (name, pt, p, "+gains" if sg else "", variant)


def matrix_inputs(case):
    """(case, args, kwargs) as inputs() gives them, the directions live_directions()' (drawn after everything else)."""
    name, pt, p, sg, variant = case
    names = sorted({c[0] for c in matrix_cases()})
    seed = 12000 + 100 * names.index(name) + 10 * pt + 2 * int(sg) + (variant == "per") + 100000 * MATRIX_RESEED.get(matrix_id(case), 0)
    c, args, kw = inputs(name, variant, MATRIX_B, MATRIX_N, p, seed)
    rng = np.random.default_rng(seed + 50000)
    dirs = live_directions(rng, c.d, p, MATRIX_B if variant == "per" else None)
    return c, args[:4] + (dirs,) + args[5:], kw


def columns(ref):
    """(smallest column maximum, smallest distance of two columns over max|ref|) of [grad_theta, grad_scale] [B, p_tot]."""
    G = np.concatenate([ref["grad_theta"]] + ([ref["grad_scale"]] if "grad_scale" in ref else []), axis=1)
    far = [np.abs(G[:, i] - G[:, j]).max() for i in range(G.shape[1]) for j in range(i)]
    return np.abs(G).max(axis=0).min(), (min(far) / np.abs(G).max() if far else np.inf)


# ---------------------------------------------------------------- the calibration's case set
class CalibrationCase:
    """Config 3's transmon (d = 3, two drives), B members whose detuning and anharmonicity (p = 2) are drawn within +-0.2 of the
    nominal scales around the nominal drift, N = 12 steps of a fixed random pulse, noise-free data from the true plants by the
    definition's own forward pass (J of the true parameters is exactly 0).  Member 0 starts at its truth; the others at the
    nominal drift.  tests/test_plant_param_host.py checks that every member converges under the definition alone."""
    B, N, p = 6, 12, 2
    GTOL, TOL, ITERS, MEM, STEPS, STEP0 = 1e-7, 0.0, 40, 5, 8, 0.25

    def __init__(self):
        c = self.c = gc.plant_case("9-2")
        rng = np.random.default_rng(20250)
        self.dirs = physical_directions(c.d)
        self.scale = np.array([0.5 * c.sat, abs(c.op0[2, 2].real)])     # what "nominal" means for the two parameters
        self.theta_true = rng.uniform(-0.2, 0.2, (self.B, self.p)) * self.scale
        self.x0 = c.states(rng, self.B)
        self.u = rng.uniform(-0.6 * c.sat, 0.6 * c.sat, (self.N, c.m))
        self.W = np.eye(c.n, dtype=complex)
        self.theta0 = np.zeros((self.B, self.p))
        self.theta0[0] = self.theta_true[0]
        self.bounds = (-0.25 * self.scale, 0.25 * self.scale)
        self._data = None

    def op0_true(self):
        return m4q.plant_param_op0(self.c.op0, self.dirs, self.theta_true)

    def data_reference(self):
        """The true plants' trajectories by the definition's forward pass (NumPy / SciPy)."""
        if self._data is None:
            from mpc4quantum_amd.plant_param import member_states
            c, o0 = self.c, self.op0_true()
            dts = np.full(self.N, c.dt)
            self._data = np.stack([member_states(self.x0[b], self.u, o0[b], c.ops, dts, c.kind) for b in range(self.B)])
        return self._data

    def args(self, data):
        c = self.c
        return (self.x0, self.u, c.op0, c.ops, self.dirs, c.dt, self.W, data)

    def kwargs(self):
        return dict(theta0=self.theta0, bounds=self.bounds, iters=self.ITERS, mem=self.MEM, steps=self.STEPS, tol=self.TOL, gtol=self.GTOL,
                    step0=self.STEP0, kind=_lib.PLANT_HAMILTONIAN)


_CAL = []


def calibration_case():
    if not _CAL:
        _CAL.append(CalibrationCase())
    return _CAL[0]

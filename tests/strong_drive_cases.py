"""Strong-drive cases of the plant kernels (tests/test_strong_drive_host.py, tests/test_gpu_strong_drive.py): seeded inputs on
tests/grad_cases.plant_case at drive levels where expm_cols (csrc/m4q_mpc.h) scales and squares, with members of one quad that
square a different number of times, and the number of squarings changing along the horizon.  No device, no library load.

squarings() mirrors expm_cols' rule (tests/test_strong_drive_host.py pins the source lines); exponents() gives, per (member, step),
the matrix whose 1-norm the device takes: the forward step's d x d exponent (Hamiltonian, process), the transposed n x n generator
(the generator plant's lane owns a ROW of L: it exponentiates L^T), and the (1 + m) d block matrix of the gradient and
linearisation kernels (csrc/m4q_grad.h).

Layouts, as every plant file's:
  shared  one operator set, one hard-driven control sequence, u_scale (small for the quiet member), a non-uniform grid,
          per-member targets
  per     the members' own operators and control sequences, no u_scale, a scalar dt, one target
A quad of five: member QUIET sees controls inside the configuration's bound (s = 0 at every step), the others see FRACTIONS of
LEVEL[cell] x sat, shaped along the horizon by ENVELOPE so that a driven member's s changes from step to step.  B = 1: the one
member is driven at the full level.  The truth of every case is tests/golden/strong_drive_truth.npz
(tests/golden/make_golden_strong_drive.py: mpmath at 40 digits).

The parameter gradient (plant_param_grad_kernel) runs on the same cases: ParamCase adds the directions, the data and the column
weights of one direction set to a Case, and param_block() is the (1 + p_tot) d matrix of param_block_expm (csrc/m4q_plant_param.h).
Its truth is tests/golden/strong_drive_param_truth.npz (tests/golden/make_golden_strong_drive_param.py)."""
import math
import os

import numpy as np

from mpc4quantum_amd import _lib
from mpc4quantum_amd.vectorize import liouvillian
from tests import grad_cases as gc
from tests import kernel_variants as kv
from tests import plant_param_cases as pc

THETA13 = 5.371920351148152              # const double theta13 = 5.371920351148152;
S_CAP = 60                               # if (s > 60) s = 60;


def squarings(norm1):
    """s of expm_cols for an exponent of 1-norm norm1:
        if (finite_d(nrm) && nrm > theta13) s = ilogb(nrm / theta13) + 1;
    ilogb(x) + 1 is the exponent frexp returns."""
    norm1 = float(norm1)
    if not math.isfinite(norm1) or not norm1 > THETA13:
        return 0
    return min(math.frexp(norm1 / THETA13)[1], S_CAP)


def norm1(Z):
    """The 1-norm as expm_cols forms it: the largest column sum of moduli."""
    return float(np.abs(Z).sum(axis=0).max())


def octave_margin(nrm):
    """|norm1 / theta13 / 2^k - 1| for the nearest power of two (inf for a norm that cannot reach theta13 by rounding): how far
    rounding of the norm is from moving s."""
    r = nrm / THETA13
    if r < 0.5:
        return math.inf
    return min(abs(r / 2.0 ** k - 1.0) for k in (math.floor(math.log2(r)), math.ceil(math.log2(r))))


# ---------------------------------------------------------------- cells
HAMILTONIAN = ("4-1", "4-2", "9-2", "16-1", "16-2", "16-3")
PROCESS = ("16-1-process", "16-2-process", "16-3-process")
GENERATOR = tuple("gen-" + name for name in HAMILTONIAN)           # every (n, m) of kv.plant_kinds with the generator plant
CELLS = HAMILTONIAN + PROCESS + GENERATOR
QP_CELLS = ("4-1", "4-2", "9-2", "16-1", "16-1-process", "16-3", "16-3-process")       # tests/test_gpu_plant_qp.py: _cells()

RUNS = [("shared", 5, 6), ("per", 5, 6), ("shared", 5, 1), ("per", 1, 1), ("shared", 1, 6)]
QUIET = 1                                                         # the quiet member of a quad of five
FRACTIONS = (1.0, None, 0.3, 0.6, 0.15)                           # the driven members' share of the level
ENVELOPE = {1: (1.0,), 6: (1.0, 0.05, 0.4, 0.012, 0.15, 0.7)}     # the drive along the horizon

# the drive level per cell, in units of the configuration's bound: the lowest of 400, 800, 1600, .. at which the preconditions of
# tests/test_strong_drive_host.py hold in every run of the cell (the process plant's dt = 0.05 needs more than the others)
LEVEL = {"4-1": 400.0, "4-2": 400.0, "9-2": 400.0, "16-1": 800.0, "16-2": 400.0, "16-3": 400.0,
         "16-1-process": 3200.0, "16-2-process": 3200.0, "16-3-process": 1600.0,
         "gen-4-1": 400.0, "gen-4-2": 400.0, "gen-9-2": 400.0, "gen-16-1": 400.0, "gen-16-2": 400.0, "gen-16-3": 400.0}


def case_id(cell, variant, B, N):
    return "%s-%s-B%d-N%d" % (cell, variant, B, N)


def all_cases(cells=CELLS):
    return [(cell, variant, B, N) for cell in cells for variant, B, N in RUNS]


def is_generator(cell):
    return cell.startswith("gen-")


def _generator_ops(c, op0, ops):
    """kv._finish's generator plant of Hamiltonian operators: the Liouvillian plus amplitude damping of the d levels."""
    a = np.diag(np.sqrt(np.arange(1, c.d)), 1).astype(complex)
    return liouvillian(op0) + 0.02 * kv.lindblad(a), np.stack([liouvillian(h) for h in ops])


class Case:
    """One run of one cell.  kind, n, m, d; x0 [B, n]; op0, ops (shared, or with a leading B); us [N, m] or [B, N, m]; u_scale
    [B, m] or None; ts (a grid, or the scalar dt); W [n, n]; f [B, n] or [n]; sat (the strong level in control units);
    v [B, N, m]: the controls each member sees; dts [N]; quiet / driven: member indices."""

    def __init__(self, cell, variant, B, N, level=None):
        c = gc.plant_case(cell[4:] if is_generator(cell) else cell)
        self.cell, self.variant, self.B, self.N, self.c = cell, variant, B, N, c
        self.level = LEVEL[cell] if level is None else level
        self.kind = _lib.PLANT_GENERATOR if is_generator(cell) else c.kind
        self.n, self.m, self.d = c.n, c.m, c.d
        rng = np.random.default_rng(7700 + 97 * CELLS.index(cell) + 11 * B + N + (500 if variant == "per" else 0))
        self.x0 = c.states(rng, B)
        self.W, f = gc.weights_and_targets(rng, c.n, B)
        frac = np.array([0.0 if fr is None else fr for fr in FRACTIONS])[:B] if B > 1 else np.array([1.0])
        self.quiet = [QUIET] if B > 1 else []
        self.driven = [b for b in range(B) if b not in self.quiet]
        env = np.array(ENVELOPE[N])[:, None]
        sign = lambda shape: rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape)
        self.sat = self.level * c.sat
        if variant == "per":
            op0, ops = c.member_ops(rng, B)
            self.us = frac[:, None, None] * self.sat * env[None] * sign((B, N, c.m))
            for b in self.quiet:
                self.us[b] = 0.5 * c.sat * env * sign((N, c.m))
            self.u_scale, self.ts, self.f = None, c.dt, f[0]
            self.v = self.us.copy()
        else:
            op0, ops = c.op0, c.ops
            self.us = self.sat * env * sign((N, c.m))
            self.u_scale = frac[:, None] * (1 + 0.1 * rng.standard_normal((B, c.m)))
            for b in self.quiet:
                self.u_scale[b] = 0.5 / self.level * (1 + 0.1 * rng.standard_normal(c.m))
            self.ts, self.f = gc.grid(rng, N, c.dt), f
            self.v = self.u_scale[:, None, :] * self.us[None]
        self.per = variant == "per"
        if is_generator(cell):
            if self.per:
                pairs = [_generator_ops(c, op0[b], ops[b]) for b in range(B)]
                op0, ops = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            else:
                op0, ops = _generator_ops(c, op0, ops)
        self.op0, self.ops = np.ascontiguousarray(op0), np.ascontiguousarray(ops)
        self.dts = np.full(N, float(self.ts)) if np.ndim(self.ts) == 0 else np.diff(self.ts)
        for a in (self.x0, self.W, self.f, self.us, self.v, self.op0, self.ops, self.dts) + (() if self.u_scale is None else (self.u_scale,)):
            a.setflags(write=False)

    @property
    def id(self):
        return case_id(self.cell, self.variant, self.B, self.N)

    def member_ops(self, b):
        return (self.op0[b], self.ops[b]) if self.per else (self.op0, self.ops)

    def target(self, b):
        return self.f[b] if self.f.ndim == 2 else self.f

    def scale(self, b):
        return np.ones(self.m) if self.u_scale is None else self.u_scale[b]

    def useq(self, b):
        return self.us[b] if self.us.ndim == 3 else self.us

    def generator(self, b, t):
        """(X, [E_k]): the exponent of member b's step t and its derivatives with respect to the controls the member sees."""
        op0, ops = self.member_ops(b)
        G = op0.astype(complex)
        for k in range(self.m):
            G = G + self.v[b, t, k] * ops[k]
        f = self.dts[t] if self.kind == _lib.PLANT_GENERATOR else -1j * self.dts[t]
        return f * G, [f * ops[k] for k in range(self.m)]

    def block(self, b, t):
        """The (1 + m) d block matrix of grad_block_expm: X on the diagonal blocks, [X, E_1 .. E_m] as the first block row."""
        X, Es = self.generator(b, t)
        d, m = X.shape[0], self.m
        Z = np.zeros(((1 + m) * d, (1 + m) * d), dtype=complex)
        for k in range(1 + m):
            Z[k * d:(k + 1) * d, k * d:(k + 1) * d] = X
        for k, E in enumerate(Es):
            Z[:d, (1 + k) * d:(2 + k) * d] = E
        return Z

    def norms(self):
        """{"forward": [B, N], "block": [B, N] (Hamiltonian and process plants)}: the 1-norms the device takes s from."""
        gen = self.kind == _lib.PLANT_GENERATOR
        out = {"forward": np.array([[norm1(self.generator(b, t)[0].T if gen else self.generator(b, t)[0]) for t in range(self.N)]
                                    for b in range(self.B)])}
        if not gen:
            out["block"] = np.array([[norm1(self.block(b, t)) for t in range(self.N)] for b in range(self.B)])
        return out

    def s(self):
        return {key: np.vectorize(squarings)(val) for key, val in self.norms().items()}

    def alone(self, b):
        """The operands of member b by itself, as a B = 1 call takes them: (x0, us, op0, ops, u_scale, f)."""
        op0, ops = self.member_ops(b)
        return (self.x0[b:b + 1], self.useq(b), op0, ops, None if self.u_scale is None else self.u_scale[b:b + 1], self.target(b))


_CASES = {}


def case(cell, variant, B, N):
    key = (cell, variant, B, N)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


# ---------------------------------------------------------------- the truth
TRUTH_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strong_drive_truth.npz")
_TRUTH = []


def truth(cs):
    """The stored truth of a case: a dict of read-only arrays (make_golden_strong_drive.py names the fields)."""
    if not _TRUTH:
        with np.load(TRUTH_FILE) as z:
            _TRUTH.append({k: z[k] for k in z.files})
        for a in _TRUTH[0].values():
            a.setflags(write=False)
    pre = cs.id + "/"
    return {k[len(pre):]: a for k, a in _TRUTH[0].items() if k.startswith(pre)}


def linearisation(cs, tr, X):
    """(A, B, Delta) at the points X [B, N, n] of a case from the truth's U and dU_k (plant_linearize.py's definition; the products
    are formed in fp64 from the fp64 roundings of the 40-digit factors)."""
    B, N, n, m, d = cs.B, cs.N, cs.n, cs.m, cs.d
    cols = 1 if cs.kind == _lib.PLANT_HAMILTONIAN else d * d
    A = np.empty((B, N, n, n), dtype=complex)
    Bm = np.empty((B, N, n, m), dtype=complex)
    Delta = np.zeros((B, N, n), dtype=complex)
    for b in range(B):
        sc, u = cs.scale(b), cs.useq(b)
        for t in range(N):
            U, dU = tr["U"][b, t], tr["dU"][b, t]
            A[b, t] = np.kron(np.kron(U, U.conj()), np.identity(cols))
            R = X[b, t].reshape(d, d, cols)
            for k in range(m):
                Bm[b, t, :, k] = sc[k] * (np.einsum('ac,cgx,eg->aex', dU[k], R, U.conj())
                                          + np.einsum('ac,cgx,eg->aex', U, R, dU[k].conj())).reshape(-1)
                Delta[b, t] -= Bm[b, t, :, k] * u[t, k]
    return A, Bm, Delta


# ---------------------------------------------------------------- the parameter gradient on the same cases
PARAM_CELLS = ("4-1", "4-2", "9-2", "16-1", "16-3", "16-1-process", "16-3-process")       # (the C entry refuses (16, 2): plant-only)
# A (case, set) whose preconditions (tests/test_strong_drive_host.py) fail on the first draw takes the next: {pair id: draws skipped}.
# 4-1-shared-B5-N1 at p = 7: the first draw's random directions lift the quiet member's block to s = 1 without any gains.
# 16-3-process-per-B1-N1 at p = 7: the one member's gradient in the first draw's direction 1 is 6.0e-4, under the 1e-3 every
# column has to exceed.
PARAM_RESEED = {"4-1-shared-B5-N1/p7": 1, "16-3-process-per-B1-N1/p7": 1}


def param_sets(cell):
    """[(p, scale_grad)] of a cell: the largest count without the gains and, where one direction or more is left, with them."""
    return [(pc.p_max(cell), False)] + ([(pc.p_max(cell, True), True)] if pc.p_max(cell, True) >= 1 else [])


def all_param_pairs(cells=PARAM_CELLS):
    return [(cell, variant, B, N, p, sg) for cell, variant, B, N in all_cases(cells) for p, sg in param_sets(cell)]


def pair_id(cell, variant, B, N, p, sg):
    return "%s/p%d%s" % (case_id(cell, variant, B, N), p, "+gains" if sg else "")


class ParamCase:
    """One direction set on one Case cs (whose controls, operators, grid and members it keeps): p directions dirs [p, d, d] (shared
    layout) or [B, p, d, d] (per), with scale_grad the m drive gains after them; data: a trajectory that is no rollout, [N + 1, n]
    or [B, N + 1, n]; col_w: zeros at columns 0, 3, 6 (shared), None (per) - as plant_param_cases.inputs."""

    def __init__(self, cs, p, sg):
        self.cs, self.p, self.sg = cs, p, sg
        self.id = pair_id(cs.cell, cs.variant, cs.B, cs.N, p, sg)
        self.p_tot = p + (cs.m if sg else 0)
        seed = 8800 + 97 * CELLS.index(cs.cell) + 11 * cs.B + cs.N + (500 if cs.per else 0) + 7 * p
        rng = np.random.default_rng(seed + 100000 * PARAM_RESEED.get(self.id, 0))
        self.dirs = pc.live_directions(rng, cs.d, p, cs.B if cs.per else None)
        self.data = pc.data_for(rng, cs.c, cs.B, cs.N, cs.per)
        self.col_w = None
        if not cs.per:
            self.col_w = rng.uniform(0.5, 1.5, cs.N + 1)
            self.col_w[::3] = 0.0
            if cs.N == 1:
                self.col_w[1] = 1.0
            self.col_w.setflags(write=False)
        self.dirs.setflags(write=False)
        self.data.setflags(write=False)

    def weights(self):
        return np.ones(self.cs.N + 1) if self.col_w is None else self.col_w

    def member_dirs(self, b):
        return self.dirs[b] if self.dirs.ndim == 4 else self.dirs

    def member_data(self, b):
        return self.data[b] if self.data.ndim == 3 else self.data

    def directions(self, b, t):
        """[E_1 .. E_p_tot] of member b's step t: -i dt D_j, then (gains) -i dt u[t][k] H_k with the UNSCALED control."""
        cs = self.cs
        f = -1j * cs.dts[t]
        Es = [f * D for D in self.member_dirs(b)]
        if self.sg:
            _, ops = cs.member_ops(b)
            Es += [f * cs.useq(b)[t, k] * ops[k] for k in range(cs.m)]
        return Es

    def param_block(self, b, t):
        """The (1 + p_tot) d matrix of param_block_expm: X on the diagonal blocks, [X, E_1 .. E_p_tot] as the first block row."""
        X, _ = self.cs.generator(b, t)
        d, n = X.shape[0], 1 + self.p_tot
        Z = np.zeros((n * d, n * d), dtype=complex)
        for k in range(n):
            Z[k * d:(k + 1) * d, k * d:(k + 1) * d] = X
        for k, E in enumerate(self.directions(b, t)):
            Z[:d, (1 + k) * d:(2 + k) * d] = E
        return Z

    def norms(self):
        """{"forward": [B, N], "param_block": [B, N]}: the 1-norms the forward and the backward pass of the kernel take s from."""
        cs = self.cs
        return {"forward": cs.norms()["forward"],
                "param_block": np.array([[norm1(self.param_block(b, t)) for t in range(cs.N)] for b in range(cs.B)])}

    def s(self):
        return {key: np.vectorize(squarings)(val) for key, val in self.norms().items()}

    def args(self):
        """(args, kwargs) of plant_param_grad_reference / plant_rollout_param_grad_batch."""
        cs = self.cs
        return ((cs.x0, cs.us, cs.op0, cs.ops, self.dirs, cs.ts, cs.W, self.data),
                dict(kind=cs.kind, u_scale=cs.u_scale, col_w=self.col_w, scale_grad=self.sg))

    def alone(self, b):
        """The same for member b by itself, as a B = 1 call takes it."""
        cs = self.cs
        x0, us, op0, ops, sc, _ = cs.alone(b)
        return ((x0, us, op0, ops, self.member_dirs(b), cs.ts, cs.W, self.member_data(b)),
                dict(kind=cs.kind, u_scale=sc, col_w=self.col_w, scale_grad=self.sg))


_PAIRS = {}


def param_case(cell, variant, B, N, p, sg):
    key = (cell, variant, B, N, p, sg)
    if key not in _PAIRS:
        _PAIRS[key] = ParamCase(case(cell, variant, B, N), p, sg)
    return _PAIRS[key]


PARAM_TRUTH_FILE = os.path.join(os.path.dirname(TRUTH_FILE), "strong_drive_param_truth.npz")
_PARAM_TRUTH = []


def param_truth(pr):
    """The stored truth of a (case, set): "J" [B], "grad_theta" [B, p] and, with the gains, "grad_scale" [B, m]."""
    if not _PARAM_TRUTH:
        with np.load(PARAM_TRUTH_FILE) as z:
            _PARAM_TRUTH.append({k: z[k] for k in z.files})
        for a in _PARAM_TRUTH[0].values():
            a.setflags(write=False)
    pre = pr.id + "/"
    return {k[len(pre):]: a for k, a in _PARAM_TRUTH[0].items() if k.startswith(pre)}
